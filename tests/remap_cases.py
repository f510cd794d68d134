"""Inputs of the rectification (cv::remap) tests, seeded, and the checks the emulator and the GPU test files share.

Source 97 x 61, destination 83 x 59 unless a case says otherwise; rows of images and maps carry padding (random bytes /
NaN) so that a kernel that ignores a stride shows.  Expected results come from tests/remap_ref.py (a restatement of OpenCV's
arithmetic, unpinned) and are computed once per (case, channels)."""
import ctypes as C
import fcntl
import functools
import os
import subprocess

import numpy as np

import remap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SRC_W, SRC_H, DST_W, DST_H = 97, 61, 83, 59
CHANNELS = (1, 3, 4)


# ---- the scalar C++ restatement (tests/remap_ref.cpp), built into tests/_build ------------------------------------------------------
@functools.lru_cache(None)
def cpp_ref():
    so, src = os.path.join(BUILD, "libremap_ref.so"), os.path.join(ROOT, "tests", "remap_ref.cpp")
    os.makedirs(BUILD, exist_ok=True)
    with open(so + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not (os.path.exists(so) and os.path.getmtime(so) >= os.path.getmtime(src)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so + ".tmp"])
            os.replace(so + ".tmp", so)
    lib = C.CDLL(so)
    lib.remap_ref.restype = C.c_int
    lib.remap_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                              C.c_int]
    return lib


def remap_cpp(img, mx, my):
    """img: (h, w[, C]) view with contiguous pixels; mx, my: float32 views sharing one row stride."""
    ch = 1 if img.ndim == 2 else img.shape[2]
    dh, dw = mx.shape
    out = np.zeros((dh, dw) if img.ndim == 2 else (dh, dw, ch), np.uint8)
    assert mx.strides == my.strides and mx.strides[1] == 4
    rc = cpp_ref().remap_ref(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], ch, mx.ctypes.data, my.ctypes.data,
                             mx.strides[0] // 4, out.ctypes.data, dw, dh, out.strides[0])
    assert rc == 0
    return out


# ---- images ------------------------------------------------------------------------------------------------------------------------
def image(channels, w=SRC_W, h=SRC_H, seed=0, pad=5, frames=1, frame_pad=0):
    """Random frames with `pad` random bytes behind every row and `frame_pad` behind every frame.
    Returns (flat uint8 buffer, row stride, frame stride, [frame views (h, w[, C])])."""
    rng = np.random.default_rng(1000 * seed + 10 * channels + w)
    stride = w * channels + pad
    fstride = stride * h + frame_pad
    buf = rng.integers(0, 256, fstride * frames, dtype=np.uint8)
    views = []
    for f in range(frames):
        rows = np.lib.stride_tricks.as_strided(buf[f * fstride:], (h, w * channels), (stride, 1))
        views.append(rows if channels == 1 else np.lib.stride_tricks.as_strided(buf[f * fstride:], (h, w, channels), (stride, channels, 1)))
    return buf, stride, fstride, views


# ---- maps --------------------------------------------------------------------------------------------------------------------------
def padded(mx, my, pad=3):
    """The two maps as views into NaN-padded buffers (map_stride_floats = width + pad)."""
    out = []
    for m in (mx, my):
        b = np.full((m.shape[0], m.shape[1] + pad), np.nan, np.float32)
        b[:, :m.shape[1]] = m
        out.append(b[:, :m.shape[1]])
    return out[0], out[1]


def grid(dw, dh):
    x, y = np.meshgrid(np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64))
    return x, y


def smooth_map(dw=DST_W, dh=DST_H, sw=SRC_W, sh=SRC_H, focal=45.0):
    """A rectification-like map: rotation by 3 degrees and radial distortion k1 = 0.35, k2 = 0.05 at focal length `focal`, about
    the centres of the two images."""
    x, y = grid(dw, dh)
    xn, yn = (x - (dw - 1) / 2) / focal, (y - (dh - 1) / 2) / focal
    a = np.deg2rad(3.0)
    xr, yr = np.cos(a) * xn - np.sin(a) * yn, np.sin(a) * xn + np.cos(a) * yn
    r2 = xr * xr + yr * yr
    d = 1 + 0.35 * r2 + 0.05 * r2 * r2
    return (focal * xr * d + (sw - 1) / 2).astype(np.float32), (focal * yr * d + (sh - 1) / 2).astype(np.float32)


def random_map(dw=DST_W, dh=DST_H, sw=SRC_W, sh=SRC_H, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-5, sw + 5, (dh, dw)).astype(np.float32), rng.uniform(-5, sh + 5, (dh, dw)).astype(np.float32))


HALF_X = [3 + 1 / 64, 3 + 3 / 64, -1 + 1 / 64, -1 / 64, -1.0, SRC_W - 1.0, SRC_W - 1 + 1 / 64, SRC_W - 2 + 63 / 64, -0.0, 96.5, -1.5, -2.0]
HALF_Y = [3 + 1 / 64, 3 + 3 / 64, -1 + 1 / 64, -1 / 64, -1.0, SRC_H - 1.0, SRC_H - 1 + 1 / 64, SRC_H - 2 + 63 / 64, -0.0, 60.5, -1.5, -2.0]
WILD = [np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38, -3e38, 2147483648.0 / 32, -2147483648.0 / 32, 67108860.0, 40000.0, -40000.0]


def base_map():
    x, y = grid(DST_W, DST_H)
    return (x + 0.25).astype(np.float32), (y + 0.5).astype(np.float32)


def halfway_map():
    """Rows 0 .. 11 x columns 0 .. 11: every pair of the half-way / border entries; the rest a plain shifted map."""
    mx, my = base_map()
    n = len(HALF_X)
    mx[:n, :n] = np.array(HALF_X, np.float32)[None, :]
    my[:n, :n] = np.array(HALF_Y, np.float32)[:, None]
    return mx, my


def wild_map():
    """Non-finite and huge entries in x (rows 0 .. 11), in y (rows 20 .. 31) and in both (rows 40 .. 51), spread over the columns."""
    mx, my = base_map()
    wild = np.array(WILD, np.float32)
    n = len(wild)
    for c in range(DST_W):
        mx[np.arange(n), c] = np.roll(wild, c)
        my[20 + np.arange(n), c] = np.roll(wild, c)
        mx[40 + np.arange(n), c] = np.roll(wild, c)
        my[40 + np.arange(n), c] = np.roll(wild, 2 * c + 1)
    return mx, my


def mixed_map():
    """Columns 0 .. 63 (the first tile column) smooth, the rest random: both kernels serve one image."""
    mx, my = smooth_map()
    rx, ry = random_map(seed=6)
    mx[:, 64:], my[:, 64:] = rx[:, 64:], ry[:, 64:]
    return mx, my


def case(name):
    """-> dict(sw, sh, mx, my): source size and the two (padded) maps."""
    sw, sh = SRC_W, SRC_H
    if name == "identity":
        x, y = grid(DST_W, DST_H)
        mx, my = x.astype(np.float32), y.astype(np.float32)
    elif name == "fractions":
        x, y = grid(32, 32)
        mx, my = (10 + x / 32).astype(np.float32), (20 + y / 32).astype(np.float32)
    elif name == "smooth":
        mx, my = smooth_map()
    elif name == "halfway":
        mx, my = halfway_map()
    elif name == "wild":
        mx, my = wild_map()
    elif name == "random":
        mx, my = random_map()
    elif name == "minify":
        sw, sh = 8 * DST_W, 8 * DST_H
        x, y = grid(DST_W, DST_H)
        mx, my = (8 * x + 3.3).astype(np.float32), (8 * y + 2.7).astype(np.float32)
    elif name == "mixed":
        mx, my = mixed_map()
    elif name == "big":
        sw, sh = 752, 480
        mx, my = smooth_map(752, 480, 752, 480, focal=45.0 * 752 / DST_W)
    else:
        raise KeyError(name)
    mx, my = padded(mx, my)
    return dict(name=name, sw=sw, sh=sh, mx=mx, my=my)


SMALL_CASES = ("identity", "fractions", "smooth", "halfway", "wild", "random", "minify", "mixed")


@functools.lru_cache(None)
def expected(name, channels, seed=0):
    """(case, source buffer, stride, source view, restated result) - computed once, never modified by the tests."""
    c = case(name)
    buf, stride, _, views = image(channels, c["sw"], c["sh"], seed=seed)
    want = R.remap(views[0], c["mx"], c["my"])
    want.setflags(write=False)
    return c, buf, stride, views[0], want


# ---- device buffers: numpy under the emulator (dev None), torch on a GPU --------------------------------------------------------------
def to_dev(a, dev):
    if dev is None:
        return a.copy()
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_ptr(t):
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def to_host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


# ---- checks shared by tests/test_remap_emu.py and tests/test_remap_gpu.py -------------------------------------------------------------
def check_host_case(lib, name, channels):
    """rgbl_remap on one case; returns the rectifier's info."""
    from orb_slam3_rgbl_amd import frontend as F
    c, _, _, view, want = expected(name, channels)
    rect = F.Rectifier(c["mx"], c["my"], (c["sw"], c["sh"]), lib=lib)
    try:
        got = rect.remap(view)
        assert got.shape == want.shape
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s C=%d: %d pixels differ, first %s" % (name, channels, len(bad), bad[:5].tolist())
        return rect.info()
    finally:
        rect.close()


def small_extractor(lib, max_batch=1):
    from orb_slam3_rgbl_amd import frontend as F
    return F.ORBextractor(300, 1.2, 2, 20, 7, 160, 128, max_batch=max_batch, lib=lib)


def check_batch_case(lib, dev, name, channels, batch):
    """rgbl_remap_batch_device on `batch` different frames with padded rows and frames; the destination's padding stays untouched."""
    from orb_slam3_rgbl_amd import frontend as F
    c = case(name)
    buf, stride, fstride, views = image(channels, c["sw"], c["sh"], seed=3, frames=batch, frame_pad=37)
    dh, dw = c["mx"].shape
    dstride = dw * channels + 7
    dfstride = dstride * dh + 13
    dst0 = np.full(dfstride * batch, 0xA5, np.uint8)
    ex = small_extractor(lib)
    rect = F.Rectifier(c["mx"], c["my"], (c["sw"], c["sh"]), lib=lib)
    try:
        d_src, d_dst = to_dev(buf, dev), to_dev(dst0, dev)
        rect.remap_batch_device(ex, dev_ptr(d_src), batch, channels, stride, fstride, dev_ptr(d_dst), dstride, dfstride)
        from orb_slam3_rgbl_amd import _lib as L
        L.check(lib, lib.rgbl_extractor_sync(ex.h))
        got = to_host(d_dst)
        for f in range(batch):
            want = R.remap(views[f], c["mx"], c["my"]).reshape(dh, dw * channels)
            rows = got[f * dfstride:f * dfstride + dstride * dh].reshape(dh, dstride)
            assert np.array_equal(rows[:, :dw * channels], want), "frame %d" % f
            assert (rows[:, dw * channels:] == 0xA5).all(), "row padding of frame %d was written" % f
            assert (got[f * dfstride + dstride * dh:(f + 1) * dfstride] == 0xA5).all(), "frame padding of frame %d was written" % f
        return rect.info()
    finally:
        rect.close()
        ex.close()


def check_errors(lib):
    """The error returns of the rectifier entry points (no kernel runs)."""
    from orb_slam3_rgbl_amd import _lib as L
    mx, my = base_map()
    h = C.c_void_p()
    P = L.ptr

    def create(sw, sh, dw, dh, x=mx, y=my, stride=DST_W):
        return lib.rgbl_rectifier_create(0, sw, sh, dw, dh, P(x) if x is not None else None, P(y) if y is not None else None, stride, C.byref(h))
    assert create(0, SRC_H, DST_W, DST_H) == L.ERR_INVALID
    assert create(SRC_W, -1, DST_W, DST_H) == L.ERR_INVALID
    assert create(SRC_W, SRC_H, 0, DST_H) == L.ERR_INVALID
    assert create(16385, SRC_H, DST_W, DST_H) == L.ERR_INVALID
    assert create(SRC_W, SRC_H, DST_W, 16385) == L.ERR_INVALID
    assert create(SRC_W, SRC_H, DST_W, DST_H, x=None) == L.ERR_INVALID
    assert create(SRC_W, SRC_H, DST_W, DST_H, y=None) == L.ERR_INVALID
    assert create(SRC_W, SRC_H, DST_W, DST_H, stride=DST_W - 1) == L.ERR_INVALID
    assert lib.rgbl_rectifier_create(0, SRC_W, SRC_H, DST_W, DST_H, P(mx), P(my), DST_W, None) == L.ERR_INVALID
    assert lib.rgbl_rectifier_create(99, SRC_W, SRC_H, DST_W, DST_H, P(mx), P(my), DST_W, C.byref(h)) == L.ERR_NO_DEVICE
    assert create(SRC_W, SRC_H, DST_W, DST_H) == L.RGBL_OK and h.value
    try:
        src = np.zeros((SRC_H, SRC_W * 4), np.uint8)
        dst = np.zeros((DST_H, DST_W * 4), np.uint8)
        assert lib.rgbl_remap(h, P(src), 2, SRC_W * 2, P(dst), DST_W * 2) == L.ERR_INVALID             # channels
        assert lib.rgbl_remap(h, P(src), 3, SRC_W * 3 - 1, P(dst), DST_W * 3) == L.ERR_INVALID         # source stride
        assert lib.rgbl_remap(h, P(src), 3, SRC_W * 3, P(dst), DST_W * 3 - 1) == L.ERR_INVALID         # destination stride
        assert lib.rgbl_remap(h, None, 1, SRC_W, P(dst), DST_W) == L.ERR_INVALID
        assert lib.rgbl_remap(None, P(src), 1, SRC_W, P(dst), DST_W) == L.ERR_INVALID
        assert lib.rgbl_remap_batch_device(h, None, P(src), 1, 1, SRC_W, 0, P(dst), DST_W, 0) == L.ERR_INVALID   # no extractor
        assert lib.rgbl_rectifier_info(None, None, None, None, None, None, None, None) == L.ERR_INVALID
        ex = small_extractor(lib)
        try:
            assert lib.rgbl_remap_batch_device(h, ex.h, P(src), 0, 1, SRC_W, 0, P(dst), DST_W, 0) == L.ERR_INVALID           # batch
            assert lib.rgbl_remap_batch_device(h, ex.h, P(src), 2, 1, SRC_W, SRC_W * SRC_H - 1, P(dst), DST_W, DST_W * DST_H) == L.ERR_INVALID
            # rgbl_extract_rectified: the rectifier's destination is not the extractor's image
            kp = np.zeros(ex.max_keypoints, L.KP_DTYPE)
            desc = np.zeros((ex.max_keypoints, 32), np.uint8)
            n, mono = C.c_int(), C.c_int()
            rc = lib.rgbl_extract_rectified(ex.h, h, P(src), 1, 0, SRC_W, SRC_H, SRC_W, 0, 0, P(kp), P(desc), len(kp), C.byref(n), C.byref(mono),
                                            None, 0)
            assert rc == L.ERR_INVALID and mono.value == -1
        finally:
            ex.close()
    finally:
        lib.rgbl_rectifier_destroy(h)


# ---- remap + cvtColor + extraction in one call ------------------------------------------------------------------------------------------
def raw_image(sw, sh, channels, seed=7):
    """A textured raw frame (the synthetic sequence of the extractor tests), colour channels made from shifted / inverted copies."""
    from orb_slam3_rgbl_amd import synth
    g = synth.Sequence(seed, sw, sh, n_frames=1).frame(0)
    if channels == 1:
        return g
    planes = [g, np.roll(g, 3, 1), 255 - np.roll(g, 2, 0), np.full_like(g, 255)]
    return np.ascontiguousarray(np.stack(planes[:channels], axis=2))


def same_keypoints(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in a.dtype.names)


def check_extract_rectified(lib, w, h, channels, nfeatures=300, nlevels=2):
    """rgbl_extract_rectified on a raw frame == rgbl_extract on the restatement's rectified (and gray-converted) frame."""
    from orb_slam3_rgbl_amd import frontend as F
    sw, sh = w + 20, h + 12
    raw = raw_image(sw, sh, channels)
    mx, my = padded(*smooth_map(w, h, sw, sh, focal=45.0 * w / DST_W))
    want = R.remap(raw, mx, my)
    want_gray = want if channels == 1 else R.cvt_gray(want, blue_first=False)
    ex = F.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, w, h, lib=lib)
    rect = F.Rectifier(mx, my, (sw, sh), lib=lib)
    try:
        for _ in range(2):   # the second call replays what the first one set up
            kps, desc, mono, gray = ex.extract_rectified(rect, raw, mbRGB=True)
            assert np.array_equal(gray, want_gray)
            k2, d2, m2 = ex(np.ascontiguousarray(want_gray))
            assert len(kps) > 50 and same_keypoints(kps, k2) and np.array_equal(desc, d2) and mono == m2
    finally:
        rect.close()
        ex.close()


def check_stereo_pair(lib, w=752, h=480):
    """A raw stereo pair through two rectifiers into rgbl_stereo_matches == the same call on host-rectified inputs."""
    from orb_slam3_rgbl_amd import frontend as F
    sw, sh = w + 20, h + 12
    left = raw_image(sw, sh, 1)
    right = np.ascontiguousarray(np.roll(left, -9, axis=1))
    mxl, myl = smooth_map(w, h, sw, sh, focal=45.0 * w / DST_W)
    mxr, myr = (mxl + np.float32(0.5)).astype(np.float32), myl.copy()
    exl, exr = (F.ORBextractor(1000, 1.2, 8, 20, 7, w, h, lib=lib) for _ in range(2))
    rl, rr = F.Rectifier(mxl, myl, (sw, sh), lib=lib), F.Rectifier(mxr, myr, (sw, sh), lib=lib)
    mb, mbf = 0.11, 47.9
    try:
        kl, dl, _, gl = exl.extract_rectified(rl, left)
        kr, dr, _, gr = exr.extract_rectified(rr, right)
        ur, dp = F.ComputeStereoMatches(exl, exr, kl, dl, kr, dr, mb, mbf)
        ur, dp = ur.copy(), dp.copy()
        hl, hr = R.remap(left, mxl, myl), R.remap(right, mxr, myr)
        assert np.array_equal(gl, hl) and np.array_equal(gr, hr)
        kl2, dl2, _ = exl(hl)
        kr2, dr2, _ = exr(hr)
        ur2, dp2 = F.ComputeStereoMatches(exl, exr, kl2, dl2, kr2, dr2, mb, mbf)
        assert same_keypoints(kl, kl2) and same_keypoints(kr, kr2)
        assert (ur2 >= 0).sum() > 50, "the pair must produce matches for the comparison to mean anything"
        assert np.array_equal(ur.view(np.uint32), ur2.view(np.uint32)) and np.array_equal(dp.view(np.uint32), dp2.view(np.uint32))
    finally:
        for o in (rl, rr, exl, exr):
            o.close()
