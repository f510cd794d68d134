"""The two cv::remap restatements (tests/remap_ref.py, tests/remap_ref.cpp) against a REAL OpenCV, wherever one is installed.
There is none in the build image, so there this file is skipped and the restatements stay unpinned (they hold each other in
tests/test_remap_restatements.py).  On a machine with OpenCV 4.x every case of tests/remap_cases.py is compared bit for bit
with cv2.remap(src, map_x, map_y, cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT, borderValue=0)."""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2")

import remap_cases as RC  # noqa: E402


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name", RC.SMALL_CASES + ("big",))
def test_restatements_match_opencv(name, channels):
    if name == "big" and channels != 1:
        pytest.skip("the full frame is a single-channel case")
    c, _, _, view, want = RC.expected(name, channels)
    mx, my = np.ascontiguousarray(c["mx"]), np.ascontiguousarray(c["my"])
    ref = cv2.remap(np.ascontiguousarray(view), mx, my, cv2.INTER_LINEAR, borderMode=cv2.BORDER_CONSTANT, borderValue=0)
    assert np.array_equal(want, ref)
    assert np.array_equal(RC.remap_cpp(view, c["mx"], c["my"]), ref)
