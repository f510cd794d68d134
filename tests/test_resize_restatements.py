"""tests/resize_ref.py (numpy, C channels) against the oracle's cv::resize (oracle/orb_oracle.cpp, scalar, one channel) and
against itself: the two are restatements of OpenCV's INTER_LINEAR arithmetic, unpinned, and must agree bit for bit; at exactly
half size the linear arithmetic IS the INTER_AREA branch OpenCV takes there, so one kernel can serve both."""
import numpy as np
import pytest

import resize_cases as RC
import resize_ref as R


@pytest.mark.parametrize("name,sizes", RC.SMALL + [("big", RC.BIG)], ids=RC.SMALL_IDS + ["big"])
def test_one_channel_equals_the_oracle(oracle, name, sizes):
    _, _, view, _ = RC.expected(sizes, 1)
    assert np.array_equal(R.resize_linear(view, sizes[2], sizes[3]), oracle.resize_linear(view, sizes[2], sizes[3]))


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name,sizes", RC.SMALL, ids=RC.SMALL_IDS)
def test_interleaved_channels_equal_the_planes(oracle, name, sizes, channels):
    _, _, view, _ = RC.expected(sizes, channels)
    got = R.resize_linear(view, sizes[2], sizes[3])
    for c in range(channels):
        assert np.array_equal(got[:, :, c], oracle.resize_linear(np.ascontiguousarray(view[:, :, c]), sizes[2], sizes[3])), "channel %d" % c


@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_half_size_linear_equals_area(channels):
    sizes = RC.CASES["half"][0]
    _, _, view, want = RC.expected(sizes, channels)
    assert R.is_area_fast(*sizes)
    assert np.array_equal(R.resize_linear(view, sizes[2], sizes[3]), R.resize_area_half(view))
    assert np.array_equal(want, R.resize_area_half(view)), "resize() takes the INTER_AREA branch here"


def test_half_size_linear_equals_area_for_every_block_sum():
    """All 2 x 2 block sums 0 .. 1020, spread over the four pixels in two ways."""
    s = np.arange(1021)
    even = np.stack([(s + k) // 4 for k in range(4)], 1)                  # a + b + c + d = s, as level as possible
    skew = np.stack([np.minimum(s, 255), np.clip(s - 255, 0, 255), np.clip(s - 510, 0, 255), np.clip(s - 765, 0, 255)], 1)
    for blocks in (even, skew):
        assert (blocks.sum(1) == s).all() and blocks.max() == 255
        img = np.zeros((2, 2 * len(s)), np.uint8)
        img[0, 0::2], img[0, 1::2], img[1, 0::2], img[1, 1::2] = blocks[:, 0], blocks[:, 1], blocks[:, 2], blocks[:, 3]
        lin = R.resize_linear(img, len(s), 1)
        assert np.array_equal(lin, R.resize_area_half(img))
        assert np.array_equal(lin[0], (s + 2) >> 2)


def test_only_half_is_area_fast():
    for name, group in RC.CASES.items():
        for sizes in group:
            assert R.is_area_fast(*sizes) == (name == "half"), (name, sizes)
    assert not R.is_area_fast(*RC.BIG)


@pytest.mark.parametrize("name,sizes", RC.SMALL + [("big", RC.BIG)], ids=RC.SMALL_IDS + ["big"])
def test_weight_pairs_sum_to_2048(name, sizes):
    sw, sh, dw, dh = sizes
    for ssize, dsize, clamp in ((sw, dw, True), (sh, dh, False)):
        s, a0, a1 = R.axis_table(ssize, dsize, clamp)
        assert ((a0 + a1) == 2048).all() and (a0 >= 0).all() and (a1 >= 0).all()
        assert s.min() >= (0 if clamp else -1) and s.max() <= ssize - 1
        if clamp:
            assert (a1[s == ssize - 1] == 0).all(), "the right tap of the last column has no weight"


def test_half_size_has_equal_weights_and_no_clamp():
    sw, sh, dw, dh = RC.CASES["half"][0]
    s, a0, a1 = R.axis_table(sw, dw, True)
    assert (a0 == 1024).all() and (a1 == 1024).all() and np.array_equal(s, 2 * np.arange(dw)) and R.clamp_counts(sw, dw) == (0, 0)


@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_same_size_returns_the_input(channels):
    sizes = RC.CASES["same"][0]
    _, _, view, want = RC.expected(sizes, channels)
    assert np.array_equal(want, view)


def test_up_case_contains_all_three_clamps():
    sw, sh, dw, dh = RC.CASES["up"][0]
    low, high = R.clamp_counts(sw, dw)
    sy, _, _ = R.axis_table(sh, dh, False)
    assert low > 0 and high > 0 and (sy == -1).sum() > 0 and (sy == sh - 1).sum() > 0
