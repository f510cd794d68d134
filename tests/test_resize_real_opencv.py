"""cv2.resize against tests/resize_ref.py on every case: the only route from "parity vs the restatement, unpinned" to a pin.
OpenCV is not part of the build image, so this skips there."""
import numpy as np
import pytest

import resize_cases as RC

cv2 = pytest.importorskip("cv2")


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name,sizes", RC.SMALL + [("big", RC.BIG)], ids=RC.SMALL_IDS + ["big"])
def test_cv2_resize_equals_the_restatement(name, sizes, channels):
    _, _, view, want = RC.expected(sizes, channels)
    got = cv2.resize(np.ascontiguousarray(view), (sizes[2], sizes[3]))
    assert np.array_equal(got.reshape(want.shape), want)
