"""Inputs of the image-resize (cv::resize) tests, seeded, and the checks the emulator and the GPU test files share.

Every case runs at 1, 3 and 4 channels with odd, unaligned strides (source w C + 3, destination dw C + 5) on random bytes with
a few rows of 0 / 255.  Expected results come from tests/resize_ref.py (a restatement of OpenCV's arithmetic = the oracle's
cv::resize at one channel, unpinned) and are computed once per (sizes, channels)."""
import ctypes as C
import functools

import numpy as np

import resize_ref as R

CHANNELS = (1, 3, 4)

# name -> [(sw, sh, dw, dh), ...]
CASES = {
    "same": [(150, 70, 150, 70)],                       # must return the input
    "euroc": [(150, 70, 120, 51)],                      # the workload's ratios (1.25 / 1.37)
    "half": [(150, 70, 75, 35)],                        # area_fast == 1; linear == 2 x 2 mean
    "near_half": [(151, 71, 75, 35)],                   # area_fast == 0
    "quarter": [(150, 70, 37, 17)],                     # taps of a 4-group far apart, tall row spans, shrunken tiles
    "up": [(150, 70, 263, 131)],                        # shared source rows; sx < 0 and sx >= sw - 1 clamps; sy = -1
    "aniso": [(150, 70, 301, 20)],                      # up in x, down 3.5 in y
    "edges": [(150, 70, 63, 31), (150, 70, 65, 33), (150, 70, 129, 17)],   # partial tiles, partial last 4-group
    "thin": [(3, 2, 7, 5), (1, 1, 5, 4), (9, 9, 1, 1)],  # sources narrower than a word, single row / column
}
SMALL = [(name, sizes) for name, group in CASES.items() for sizes in group]
SMALL_IDS = ["%s-%dx%d-%dx%d" % ((name,) + sizes) for name, sizes in SMALL]
BIG = (752, 480, 600, 350)
BATCH_CASE = CASES["euroc"][0]


# ---- images ------------------------------------------------------------------------------------------------------------------------
def image(channels, w, h, seed=0, pad=3, frames=1, frame_pad=0):
    """Random frames with `pad` random bytes behind every row and `frame_pad` behind every frame; rows 1 / 2 (where they exist)
    and the last row of every frame are all 0 / all 255 / all 255.  Returns (flat buffer, row stride, frame stride, [views])."""
    rng = np.random.default_rng(1000 * seed + 10 * channels + w)
    stride = w * channels + pad
    fstride = stride * h + frame_pad
    buf = rng.integers(0, 256, fstride * frames, dtype=np.uint8)
    views = []
    for f in range(frames):
        rows = np.lib.stride_tricks.as_strided(buf[f * fstride:], (h, w * channels), (stride, 1))
        if h > 3:
            rows[1], rows[2], rows[h - 1] = 0, 255, 255
        views.append(rows if channels == 1 else np.lib.stride_tricks.as_strided(buf[f * fstride:], (h, w, channels), (stride, channels, 1)))
    return buf, stride, fstride, views


@functools.lru_cache(None)
def expected(sizes, channels, seed=0):
    """(source buffer, stride, source view, restated result) - computed once, never modified by the tests."""
    sw, sh, dw, dh = sizes
    buf, stride, _, views = image(channels, sw, sh, seed=seed)
    want = R.resize(views[0], dw, dh)
    want.setflags(write=False)
    buf.setflags(write=False)
    return buf, stride, views[0], want


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


# ---- checks shared by tests/test_resize_emu.py and tests/test_resize_gpu.py -----------------------------------------------------------
def check_host_case(lib, sizes, channels):
    """rgbl_resize on one case with the strides w C + 3 / dw C + 5; the destination's padding stays untouched.  Returns the info."""
    from orb_slam3_rgbl_amd import _lib as L
    from orb_slam3_rgbl_amd import frontend as F
    sw, sh, dw, dh = sizes
    buf, stride, _, want = expected(sizes, channels)
    dstride = dw * channels + 5
    dst = np.full(dstride * dh, 0xA5, np.uint8)
    rs = F.Resizer((sw, sh), (dw, dh), lib=lib)
    try:
        L.check(lib, lib.rgbl_resize(rs.h, L.ptr(buf), channels, stride, L.ptr(dst), dstride))
        rows = dst.reshape(dh, dstride)
        got = rows[:, :dw * channels].reshape(want.shape)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s C=%d: %d bytes differ, first %s" % (sizes, channels, len(bad), bad[:5].tolist())
        assert (rows[:, dw * channels:] == 0xA5).all(), "row padding was written"
        info = rs.info()
        assert (info["src_w"], info["src_h"], info["dst_w"], info["dst_h"]) == sizes
        return info
    finally:
        rs.close()


def small_extractor(lib, max_batch=1):
    from orb_slam3_rgbl_amd import frontend as F
    return F.ORBextractor(300, 1.2, 2, 20, 7, 160, 128, max_batch=max_batch, lib=lib)


def check_batch_case(lib, dev, channels, batch):
    """rgbl_resize_batch_device on `batch` different frames with padded rows and frames; the destination's padding stays untouched."""
    from orb_slam3_rgbl_amd import _lib as L
    from orb_slam3_rgbl_amd import frontend as F
    sw, sh, dw, dh = BATCH_CASE
    buf, stride, fstride, views = image(channels, sw, sh, seed=3, frames=batch, frame_pad=37)
    dstride = dw * channels + 5
    dfstride = dstride * dh + 13
    dst0 = np.full(dfstride * batch, 0xA5, np.uint8)
    ex = small_extractor(lib, max_batch=batch)
    rs = F.Resizer((sw, sh), (dw, dh), lib=lib)
    try:
        d_src, d_dst = to_dev(buf, dev), to_dev(dst0, dev)
        rs.resize_batch_device(ex, dev_ptr(d_src), batch, channels, stride, fstride, dev_ptr(d_dst), dstride, dfstride)
        L.check(lib, lib.rgbl_extractor_sync(ex.h))
        got = to_host(d_dst)
        for f in range(batch):
            want = R.resize(views[f], dw, dh).reshape(dh, dw * channels)
            rows = got[f * dfstride:f * dfstride + dstride * dh].reshape(dh, dstride)
            assert np.array_equal(rows[:, :dw * channels], want), "frame %d" % f
            assert (rows[:, dw * channels:] == 0xA5).all(), "row padding of frame %d was written" % f
            assert (got[f * dfstride + dstride * dh:(f + 1) * dfstride] == 0xA5).all(), "frame padding of frame %d was written" % f
    finally:
        rs.close()
        ex.close()


def check_errors(lib):
    """The error returns of the resizer entry points (no kernel runs)."""
    from orb_slam3_rgbl_amd import _lib as L
    sw, sh, dw, dh = 97, 61, 83, 59
    h = C.c_void_p()
    P = L.ptr

    def failed(rc, code=L.ERR_INVALID):
        return rc == code and len(lib.rgbl_last_error()) > 0
    for bad in [(0, sh, dw, dh), (sw, -1, dw, dh), (sw, sh, 0, dh), (sw, sh, dw, 0), (16385, sh, dw, dh), (sw, 16385, dw, dh), (sw, sh, 16385, dh),
                (sw, sh, dw, 16385)]:
        assert failed(lib.rgbl_resizer_create(0, *bad, C.byref(h))) and not h.value
    assert failed(lib.rgbl_resizer_create(0, sw, sh, dw, dh, None))
    assert failed(lib.rgbl_resizer_create(99, sw, sh, dw, dh, C.byref(h)), L.ERR_NO_DEVICE)
    assert lib.rgbl_resizer_create(0, sw, sh, dw, dh, C.byref(h)) == L.RGBL_OK and h.value
    try:
        src = np.zeros((sh, sw * 4), np.uint8)
        dst = np.zeros((dh, dw * 4), np.uint8)
        assert failed(lib.rgbl_resize(h, P(src), 2, sw * 2, P(dst), dw * 2))               # channels
        assert failed(lib.rgbl_resize(h, P(src), 3, sw * 3 - 1, P(dst), dw * 3))           # source stride
        assert failed(lib.rgbl_resize(h, P(src), 3, sw * 3, P(dst), dw * 3 - 1))           # destination stride
        assert failed(lib.rgbl_resize(h, None, 1, sw, P(dst), dw))
        assert failed(lib.rgbl_resize(h, P(src), 1, sw, None, dw))
        assert failed(lib.rgbl_resize(None, P(src), 1, sw, P(dst), dw))
        assert failed(lib.rgbl_resize_batch_device(h, None, P(src), 1, 1, sw, 0, P(dst), dw, 0))   # no extractor
        assert failed(lib.rgbl_resizer_info(None, None, None, None, None, None, None))
        assert not dst.any(), "a refused call must not write"
        ex = small_extractor(lib, max_batch=2)
        try:
            assert failed(lib.rgbl_resize_batch_device(h, ex.h, P(src), 0, 1, sw, 0, P(dst), dw, 0))                   # batch < 1
            assert failed(lib.rgbl_resize_batch_device(h, ex.h, P(src), 3, 1, sw, sw * sh, P(dst), dw, dw * dh))       # above max_batch
            assert failed(lib.rgbl_resize_batch_device(h, ex.h, P(src), 2, 1, sw, sw * sh - 1, P(dst), dw, dw * dh))   # frames overlap
            assert failed(lib.rgbl_resize_batch_device(h, ex.h, P(src), 1, 5, sw * 5, 0, P(dst), dw * 5, 0))           # channels
            assert failed(lib.rgbl_resize_batch_device(h, ex.h, None, 1, 1, sw, 0, P(dst), dw, 0))
            assert failed(lib.rgbl_resize_batch_device(h, ex.h, P(src), 1, 1, sw, 0, None, dw, 0))
            # rgbl_extract_resized: the resizer's destination is not the extractor's image
            kp = np.zeros(ex.max_keypoints, L.KP_DTYPE)
            desc = np.zeros((ex.max_keypoints, 32), np.uint8)
            n, mono = C.c_int(), C.c_int()
            rc = lib.rgbl_extract_resized(ex.h, h, P(src), 1, 0, sw, sh, sw, 0, 0, P(kp), P(desc), len(kp), C.byref(n), C.byref(mono), None, 0)
            assert failed(rc) and mono.value == -1
        finally:
            ex.close()
    finally:
        lib.rgbl_resizer_destroy(h)


# ---- resize + cvtColor + extraction in one call -------------------------------------------------------------------------------------------
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


def check_extract_resized(lib, sw, sh, w, h, channels, nfeatures=300, nlevels=2):
    """rgbl_extract_resized on a raw frame == rgbl_extract on the restatement's resized, THEN gray-converted frame."""
    from orb_slam3_rgbl_amd import frontend as F
    raw = raw_image(sw, sh, channels)
    want = R.resize(raw, w, h)
    want_gray = want if channels == 1 else R.cvt_gray(want, blue_first=False)
    ex = F.ORBextractor(nfeatures, 1.2, nlevels, 20, 7, w, h, lib=lib)
    rs = F.Resizer((sw, sh), (w, h), lib=lib)
    try:
        for _ in range(2):   # the second call replays what the first one set up
            kps, desc, mono, gray = ex.extract_resized(rs, raw, mbRGB=True)
            assert np.array_equal(gray, want_gray)
            k2, d2, m2 = ex(np.ascontiguousarray(want_gray))
            assert len(kps) > 50 and same_keypoints(kps, k2) and np.array_equal(desc, d2) and mono == m2
    finally:
        rs.close()
        ex.close()


def check_stereo_pair(lib, sw=752, sh=480, w=600, h=350):
    """A raw stereo pair through two rgbl_extract_resized calls into rgbl_stereo_matches == the same call on restated images."""
    from orb_slam3_rgbl_amd import frontend as F
    left = raw_image(sw, sh, 1)
    right = np.ascontiguousarray(np.roll(left, -11, axis=1))
    exl, exr = (F.ORBextractor(1000, 1.2, 8, 20, 7, w, h, lib=lib) for _ in range(2))
    rs = F.Resizer((sw, sh), (w, h), lib=lib)
    mb, mbf = 0.11, 47.9
    try:
        kl, dl, _, gl = exl.extract_resized(rs, left)
        kr, dr, _, gr = exr.extract_resized(rs, right)
        ur, dp = F.ComputeStereoMatches(exl, exr, kl, dl, kr, dr, mb, mbf)
        ur, dp = ur.copy(), dp.copy()
        hl, hr = R.resize(left, w, h), R.resize(right, w, h)
        assert np.array_equal(gl, hl) and np.array_equal(gr, hr)
        kl2, dl2, _ = exl(hl)
        kr2, dr2, _ = exr(hr)
        ur2, dp2 = F.ComputeStereoMatches(exl, exr, kl2, dl2, kr2, dr2, mb, mbf)
        assert same_keypoints(kl, kl2) and same_keypoints(kr, kr2)
        assert (ur2 >= 0).sum() > 50, "the pair must produce matches for the comparison to mean anything"
        assert np.array_equal(ur.view(np.uint32), ur2.view(np.uint32)) and np.array_equal(dp.view(np.uint32), dp2.view(np.uint32))
    finally:
        for o in (rs, exl, exr):
            o.close()
