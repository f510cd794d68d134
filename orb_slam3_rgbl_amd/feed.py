"""Host-fed batches: the Python mirror of the library's rgbl_feeder (include/rgbl_frontend.h, csrc/feed.hip).

A real RGB-L run reads every frame into host memory - a colour PNG and a velodyne .bin scan, one frame after another
(Examples/RGB-L/rgbl_kitti.cc:87-94, 151-185).  A `HostFeeder` takes those frames in batches through page-locked slots: the
numpy views it hands out ARE the page-locked memory, so `np.fromfile(path, np.float32)` (through `scan_view`) or a decoder
writes straight into the slot, and `submit()` queues the copies and the whole front end (cvtColor, ORB extraction,
UndistortKeyPoints, CalculateDepthFromPcd) without waiting.  `run(frames)` keeps `slots` batches in flight.

    fd = HostFeeder(extractor, depth, channels=3, blue_first=1, max_batch=64, max_points=130000, slots=3)
    for frames in fd.run(batches):        # batches: iterable of lists of (image, xyzi) pairs
        for fr in frames: fr["kp"], fr["desc"], fr["depth"], fr["uright"], ...
"""
import ctypes as C

import numpy as np

from . import _lib as L


class HostFeeder:
    def __init__(self, extractor, depth, channels=3, blue_first=1, max_batch=1, max_points=130000, max_points_batch=0,
                 slots=3, K=None, dist=None, lib=None):
        """extractor / depth: frontend.ORBextractor / frontend.DepthModule (or anything with .h and .lib).  K = (fx, fy, cx,
        cy) and dist = (k1, k2, p1, p2[, k3]) switch UndistortKeyPoints on when dist[0] != 0 (Frame.cc:839)."""
        self.lib = lib or extractor.lib
        cfg = L.FeederCfg()
        cfg.channels, cfg.blue_first, cfg.max_batch, cfg.max_points = channels, int(bool(blue_first)), max_batch, max_points
        cfg.max_points_batch, cfg.slots = max_points_batch, slots
        if dist is not None and len(dist):
            if K is None or len(K) != 4:
                raise ValueError("undistortion needs K = (fx, fy, cx, cy) next to dist")
            for i, v in enumerate(K):
                cfg.K[i] = float(v)
            for i, v in enumerate(dist):
                cfg.dist[i] = float(v)
            cfg.n_dist = len(dist)
        self.cfg = cfg
        self.ex, self.dm = extractor, depth  # the handles must outlive the feeder
        self.h = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_feeder_create(C.byref(cfg), extractor.h, depth.h, C.byref(self.h)))
        self.w, self.height = depth.cfg.width, depth.cfg.height
        self.channels, self.max_batch, self.slots = channels, max_batch, slots
        self.pinned_bytes = int(self.lib.rgbl_feeder_pinned_bytes(self.h))
        self.undistort = cfg.n_dist > 0 and cfg.dist[0] != 0.0

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.rgbl_feeder_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the protocol, one call each ----
    def acquire(self):
        s = C.c_int()
        L.check(self.lib, self.lib.rgbl_feeder_acquire(self.h, C.byref(s)))
        return s.value

    def image_view(self, slot, b):
        """Frame b's image in the page-locked slot: (h, w) or (h, w, channels) uint8, written in place."""
        p = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_feeder_image(self.h, slot, b, C.byref(p)))
        shape = (self.height, self.w) if self.channels == 1 else (self.height, self.w, self.channels)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=shape)

    def scan_view(self, slot, b, n):
        """Reserves n .bin records for frame b (frames in order) and returns them as an (n, 4) float32 view."""
        p = C.c_void_p()
        L.check(self.lib, self.lib.rgbl_feeder_scan(self.h, slot, b, int(n), C.byref(p)))
        if n == 0:
            return np.zeros((0, 4), np.float32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(int(n), 4))

    def fill(self, slot, b, image, xyzi):
        """Copies one frame into the slot: image (h, w[, channels]) uint8, xyzi (n, 4) float32 or the flat .bin array."""
        pts = np.asarray(xyzi, np.float32).reshape(-1, 4)
        self.scan_view(slot, b, len(pts))[...] = pts
        self.image_view(slot, b)[...] = np.asarray(image, np.uint8).reshape(self.image_view(slot, b).shape)

    def submit(self, slot, batch):
        L.check(self.lib, self.lib.rgbl_feeder_submit(self.h, slot, batch))

    def collect_raw(self, slot):
        """Waits for the slot's batch; (status, rgbl_feeder_results) - status != 0 is a deferred device error."""
        r = L.FeederResults()
        rc = self.lib.rgbl_feeder_collect(self.h, slot, C.byref(r))
        return rc, r

    def collect(self, slot):
        """Waits for the slot's batch and returns one dict per frame (copies): kp (KP_DTYPE), desc (n x 32), depth,
        uright, mono and kpun_xy (n x 2, only when undistorting)."""
        rc, r = self.collect_raw(slot)
        L.check(self.lib, rc)
        return self.frames(r)

    def device_outputs(self, slot):
        """(rgbl_feeder_results with device pointers, done event as c_void_p)."""
        r, ev = L.FeederResults(), C.c_void_p()
        L.check(self.lib, self.lib.rgbl_feeder_device_outputs(self.h, slot, C.byref(r), C.byref(ev)))
        return r, ev

    @staticmethod
    def _arr(p, ctype, shape):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=shape)

    def frames(self, r):
        B, cap = r.batch, r.cap
        n = self._arr(r.n, C.c_int32, (B,)).copy()
        mono = self._arr(r.mono, C.c_int32, (B,)).copy()
        kp = self._arr(r.kp, C.c_uint8, (B, cap * 28)).view(L.KP_DTYPE)
        desc = self._arr(r.desc, C.c_uint8, (B, cap, 32))
        depth = self._arr(r.depth, C.c_float, (B, cap))
        ur = self._arr(r.uright, C.c_float, (B, cap))
        un = self._arr(r.kpun_xy, C.c_float, (B, cap, 2)) if r.kpun_xy else None
        out = []
        for b in range(B):
            k = int(n[b])
            fr = dict(n=k, mono=int(mono[b]), kp=kp[b, :k].copy(), desc=desc[b, :k].copy(), depth=depth[b, :k].copy(),
                      uright=ur[b, :k].copy())
            if un is not None:
                fr["kpun_xy"] = un[b, :k].copy()
            out.append(fr)
        return out

    def run(self, batches):
        """Generator: for every batch (a list of (image, xyzi) pairs, at most max_batch) the list of per-frame result dicts,
        in order, with up to `slots` batches in flight."""
        pending = []
        for frames in batches:
            if len(pending) == self.slots:
                yield self.collect(pending.pop(0))
            s = self.acquire()
            for b, (img, pts) in enumerate(frames):
                self.fill(s, b, img, pts)
            self.submit(s, len(frames))
            pending.append(s)
        while pending:
            yield self.collect(pending.pop(0))
