"""cv::remap(src, dst, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit images with CV_32FC1 maps, restated in
vectorised numpy from the published OpenCV 4.x algorithm (imgproc/src/remap.cpp).  No OpenCV is installed in the build
image, so this is a restatement, unpinned; tests/remap_ref.cpp is a second one written independently (scalar C++, OpenCV's
15-bit weight table and its three border branches) and tests/test_remap_restatements.py holds the two against each other.

Formulation here: every output pixel takes four taps with 10-bit weights, every tap is tested against the image on its
own, result = (sum + 512) >> 10."""
import numpy as np


def fixed_point(m):
    """cvRound(m * 32): fp32 product, half-to-even; NaN and |v| >= 2^31 give INT32_MIN (x86 cvtss2si)."""
    with np.errstate(all="ignore"):
        v = np.asarray(m, np.float32) * np.float32(32)
        bad = ~(np.abs(v) < np.float32(2147483648.0))
        s = np.rint(np.where(bad, np.float32(0), v)).astype(np.int64)
    s[bad] = -(1 << 31)
    return s


def coordinates(mx, my):
    """(ix, iy, fx, fy): saturate_cast<short>(s >> 5) and s & 31 of both axes."""
    sx, sy = fixed_point(mx), fixed_point(my)
    return np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767), sx & 31, sy & 31


def taps_inside(mx, my, sw, sh):
    """How many of the four taps of every output pixel lie inside a sw x sh source (0 .. 4)."""
    ix, iy, _, _ = coordinates(mx, my)
    n = np.zeros(ix.shape, np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            n += ((ix + dx >= 0) & (ix + dx < sw) & (iy + dy >= 0) & (iy + dy < sh))
    return n


def remap(src, mx, my):
    """src: (h, w) or (h, w, C) uint8; mx, my: (dh, dw) float32.  Returns (dh, dw[, C]) uint8."""
    S = src[:, :, None] if src.ndim == 2 else src
    sh, sw, _ = S.shape
    S = S.astype(np.int64)
    ix, iy, fx, fy = coordinates(mx, my)

    def tap(r, q):
        ok = (q >= 0) & (q < sw) & (r >= 0) & (r < sh)
        v = S[np.clip(r, 0, sh - 1), np.clip(q, 0, sw - 1)]
        return np.where(ok[:, :, None], v, 0)

    w00, w01, w10, w11 = (32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy
    acc = (tap(iy, ix) * w00[:, :, None] + tap(iy, ix + 1) * w01[:, :, None] + tap(iy + 1, ix) * w10[:, :, None] +
           tap(iy + 1, ix + 1) * w11[:, :, None] + 512) >> 10
    out = acc.astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def cvt_gray(img, blue_first):
    """cv::cvtColor(COLOR_{BGR,RGB}[A]2GRAY), OpenCV 4.x: 15-bit weights R 9798, G 19235, B 3735."""
    c = img.astype(np.int64)
    w0, w2 = (3735, 9798) if blue_first else (9798, 3735)
    return ((c[:, :, 0] * w0 + c[:, :, 1] * 19235 + c[:, :, 2] * w2 + (1 << 14)) >> 15).astype(np.uint8)
