"""cv::remap (INTER_LINEAR, CV_32FC1 maps, BORDER_CONSTANT 0, 8-bit) cannot be checked against a real OpenCV in the build image,
so - as tests/test_opencv_restatements.py does for the extractor's primitives - two restatements written independently must
agree bit for bit on every case of tests/remap_cases.py: the vectorised numpy one (tests/remap_ref.py: 10-bit weights, every
tap tested on its own) and the scalar C++ one (tests/remap_ref.cpp: OpenCV's 15-bit `short` table, cvtss2si, the three
border branches).  Parity of everything else is stated against these restatements, unpinned."""
import numpy as np
import pytest

import remap_cases as RC
import remap_ref as R


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name", RC.SMALL_CASES)
def test_two_restatements_agree(name, channels):
    c, _, _, view, want = RC.expected(name, channels)
    assert np.array_equal(RC.remap_cpp(view, c["mx"], c["my"]), want)


def test_two_restatements_agree_on_a_full_frame():
    c, _, _, view, want = RC.expected("big", 1)
    assert np.array_equal(RC.remap_cpp(view, c["mx"], c["my"]), want)


@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_identity_map_returns_the_input(channels):
    _, _, _, view, want = RC.expected("identity", channels)
    assert np.array_equal(want, view[:RC.DST_H, :RC.DST_W])


def test_fraction_sweep_covers_all_1024_pairs():
    c = RC.case("fractions")
    _, _, fx, fy = R.coordinates(c["mx"], c["my"])
    assert len(set(zip(fx.ravel().tolist(), fy.ravel().tolist()))) == 1024


def test_fifteen_bit_and_ten_bit_weights_agree_for_every_fraction_pair():
    """(sum tap * 32 w + 2^14) >> 15 == (sum tap * w + 512) >> 10, and the saturated (0, 0) weight 32767 changes nothing."""
    v = np.arange(256, dtype=np.int64)
    assert np.array_equal((v * 32767 + (1 << 14)) >> 15, v)
    rng = np.random.default_rng(0)
    t = rng.integers(0, 256, (4, 4096), dtype=np.int64)
    for fy in range(32):
        for fx in range(32):
            w = np.array([(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy], np.int64)[:, None]
            assert w.sum() == 1024
            assert np.array_equal(((t * w * 32).sum(0) + (1 << 14)) >> 15, ((t * w).sum(0) + 512) >> 10)


def test_smooth_map_has_every_border_class():
    c = RC.case("smooth")
    n = R.taps_inside(c["mx"], c["my"], c["sw"], c["sh"])
    assert (n == 0).sum() > 0 and (n == 2).sum() > 0 and (n == 1).sum() > 0 and (n == 4).sum() > 0
    ix, iy, _, _ = R.coordinates(c["mx"], c["my"])
    part = (n > 0) & (n < 4)
    for side in (ix == -1, ix == c["sw"] - 1, iy == -1, iy == c["sh"] - 1):   # partial pixels on all four borders
        assert (part & side).any()


def test_half_way_roundings():
    s = R.fixed_point(np.float32([3 + 1 / 64, 3 + 3 / 64, -1 + 1 / 64, -1 / 64]))
    assert s.tolist() == [96, 98, -32, 0]


def test_non_finite_and_huge_entries_give_zero():
    s = R.fixed_point(np.float32([np.nan, np.inf, -np.inf, 1e9, -1e9, 3e38, -3e38]))
    assert (s == -(1 << 31)).all()
    for channels in RC.CHANNELS:
        c, _, _, _, want = RC.expected("wild", channels)
        wild = ~np.isfinite(c["mx"]) | ~np.isfinite(c["my"]) | (np.abs(c["mx"]) >= 3e4) | (np.abs(c["my"]) >= 3e4)
        assert wild.sum() >= 3 * 12 * RC.DST_W and (want[wild] == 0).all()
