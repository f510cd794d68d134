"""rgbl_map_points_refresh on a real MI355X: the checks of tests/map_refresh_checks.py on the product library
(tests/test_map_refresh_emu.py runs them under the emulator), and a map of KITTI size."""
import pytest

import map_refresh_checks as mr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_kfs", mr.KF_COUNTS)
def test_every_size_against_restatement_and_oracle(gpu_lib, n_kfs):
    assert mr.check_sizes(gpu_lib, n_kfs) == sum(mr.POINT_COUNTS) * sum(mr.OBS_COUNTS)


def test_rules_of_the_two_reference_functions(gpu_lib):
    mr.check_rules(gpu_lib)


def test_wide_range_of_magnitudes_and_a_point_on_a_camera_centre(gpu_lib):
    """the device's fp64-routed square root and division against the host's fp32 ones"""
    mr.check_wide_range(gpu_lib)


def test_track_local_points_on_the_refreshed_pool(gpu_lib):
    assert mr.check_track_after_refresh(gpu_lib) > 10


def test_error_returns_leave_the_pool_unchanged(gpu_lib):
    mr.check_errors(gpu_lib)


def test_refresh_next_to_search_and_update(gpu_lib):
    mr.check_threads(gpu_lib)


def test_kitti_sized_map(gpu_lib):
    """1 500 points, 40 key frames of 2 000 features, about 15 observations each (what tools/map_refresh_bench.py times)."""
    mr.check_kitti_size(gpu_lib)
