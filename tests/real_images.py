"""Real photographs for rows f1 / f3, scikit-image sample data stored under tests/golden/photos
(tests/golden/README.md lists where each comes from):
  motorcycle_left.png / motorcycle_right.png  a rectified stereo pair (Middlebury 2014 'Motorcycle', 741 x 500 RGB) with its
                                              ground-truth disparity motorcycle_disp.npy.xz - Frame::ComputeStereoMatches (Frame.cc:901-1071)
  astronaut.png, coffee.png                   colour photographs - cvtColor -> extract (Tracking.cc:1567-1580)
"""
import io
import lzma
import os

import numpy as np
import pytest

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photos")


def _rgb(name):
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("PIL is not importable here")
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(DATA, name)).convert("RGB"), np.uint8))


def stereo_pair():
    """(left RGB, right RGB, ground-truth disparity of the left view [h, w] float32, inf where unknown)."""
    left, right = _rgb("motorcycle_left.png"), _rgb("motorcycle_right.png")
    with open(os.path.join(DATA, "motorcycle_disp.npy.xz"), "rb") as f:
        disp = np.load(io.BytesIO(lzma.decompress(f.read()))).astype(np.float32)
    return left, right, disp


def color_photo(name="astronaut.png"):
    return _rgb(name)


# camera of the skimage copy of the Middlebury pair: focal length 3979.911 px and baseline 193.001 mm at 2964 x 1988, scaled to 741 x 500
MOTORCYCLE_FX = 3979.911 * 741.0 / 2964.0
MOTORCYCLE_MB = 0.193001
MOTORCYCLE_MBF = MOTORCYCLE_FX * MOTORCYCLE_MB
