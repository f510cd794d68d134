"""cv::resize(src, dst, dsize) on 8-bit images with 1, 3 or 4 interleaved channels, restated in vectorised numpy from the
published OpenCV 4.x algorithm (imgproc/src/resize.cpp).  No OpenCV is installed in the build image, so this is a restatement,
unpinned; at one channel oracle/orb_oracle.cpp holds a second one written independently (scalar C++), and
tests/test_resize_restatements.py holds the two against each other.

resize_linear is the default INTER_LINEAR in 11-bit fixed point, every channel on its own.  resize_area_half is what OpenCV
computes instead at exactly half size (INTER_LINEAR && is_area_fast && iscale_x == 2 && iscale_y == 2 -> INTER_AREA):
the rounded 2 x 2 mean.  resize() takes the branch OpenCV takes; the two give the same bytes (the restatement tests say so)."""
import numpy as np

COEF = 2048   # INTER_RESIZE_COEF_SCALE


def axis_table(ssize, dsize, clamp):
    """(s, a0, a1) of one axis: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; with `clamp` (the x axis)
    s < 0 -> (0, f = 0) and s >= ssize - 1 -> (ssize - 1, f = 0).  Weights cvRound((1 - f) * 2048), cvRound(f * 2048)."""
    scale = 1.0 / (float(dsize) / float(ssize))                      # double, as OpenCV computes it from inv_scale
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp:
        low, high = s < 0, s >= ssize - 1
        s = np.where(low, 0, np.where(high, ssize - 1, s))
        f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f) * np.float32(COEF)).astype(np.int64)   # half to even, as cvRound
    a1 = np.rint(f * np.float32(COEF)).astype(np.int64)
    return s, a0, a1


def clamp_counts(ssize, dsize):
    """How many x entries the two clamps caught: (s < 0, s >= ssize - 1), before clamping."""
    scale = 1.0 / (float(dsize) / float(ssize))
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return int((s < 0).sum()), int((s >= ssize - 1).sum())


def is_area_fast(sw, sh, dw, dh):
    """resize.cpp: the half-size case that INTER_LINEAR hands to INTER_AREA."""
    eps = np.finfo(np.float64).eps
    sx, sy = 1.0 / (float(dw) / sw), 1.0 / (float(dh) / sh)
    return abs(sx - 2.0) < eps and abs(sy - 2.0) < eps


def resize_linear(src, dw, dh):
    """src: (h, w) or (h, w, C) uint8 -> (dh, dw[, C]) uint8, INTER_LINEAR."""
    S = (src[:, :, None] if src.ndim == 2 else src).astype(np.int64)
    sh, sw, _ = S.shape
    sx, a0, a1 = axis_table(sw, dw, True)
    sy, b0, b1 = axis_table(sh, dh, False)
    sx1 = np.minimum(sx + 1, sw - 1)                                   # its weight is 0 wherever sx is the last column
    H = S[:, sx, :] * a0[None, :, None] + S[:, sx1, :] * a1[None, :, None]   # the horizontal pass of every source row
    r0, r1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    out = (((b0[:, None, None] * (H[r0] >> 4)) >> 16) + ((b1[:, None, None] * (H[r1] >> 4)) >> 16) + 2) >> 2
    out = (out & 0xff).astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def resize_area_half(src):
    """INTER_AREA at scale 2 x 2 (resizeAreaFast): (a + b + c + d + 2) >> 2 of every 2 x 2 block; even sides."""
    S = (src[:, :, None] if src.ndim == 2 else src).astype(np.int64)
    assert S.shape[0] % 2 == 0 and S.shape[1] % 2 == 0
    out = ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def resize(src, dw, dh):
    """cv::resize(src, dst, Size(dw, dh)) as OpenCV routes it."""
    sh, sw = src.shape[:2]
    if is_area_fast(sw, sh, dw, dh):
        return resize_area_half(src)
    return resize_linear(src, dw, dh)


def cvt_gray(img, blue_first):
    """cv::cvtColor(COLOR_{BGR,RGB}[A]2GRAY), OpenCV 4.x: 15-bit weights R 9798, G 19235, B 3735."""
    c = img.astype(np.int64)
    w0, w2 = (3735, 9798) if blue_first else (9798, 3735)
    return ((c[:, :, 0] * w0 + c[:, :, 1] * 19235 + c[:, :, 2] * w2 + (1 << 14)) >> 15).astype(np.uint8)
