"""rgbl_create_new_map_points / rgbl_triangulate_matches on a real MI355X: the checks of tests/new_points_checks.py on the
product library (tests/test_new_points_emu.py runs them under the emulator), the device's atan2f / cosf restatement against the
host's, and a key frame of KITTI size."""
import ctypes as C

import numpy as np
import pytest

import new_points_checks as nc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_neigh", nc.NEIGHBOUR_COUNTS)
def test_every_size_against_the_restatement(gpu_lib, n_neigh):
    total = nc.check_sizes(gpu_lib, n_neigh)
    assert (total > 100) == (n_neigh > 0)


def test_main_fixture_chain_and_status_coverage(gpu_lib):
    counts = nc.check_main(gpu_lib)
    assert all(counts[s] >= 3 for s in nc.STATUSES_IN_FIXTURE)


def test_more_matches_than_one_tile_in_one_launch(gpu_lib):
    assert nc.check_dense(gpu_lib) > 512


@pytest.mark.parametrize("name", ["inertial", "main", "monocular"])
def test_device_matches_the_reference_fixtures(gpu_lib, name):
    """tests/golden/new_points: what the reference's own CreateNewMapPoints left in mlpRecentAddedMapPoints (tests/new_points_golden.py)"""
    import new_points_golden as ng
    from orb_slam3_rgbl_amd import frontend as F
    mt = F.ORBmatcher(0.6, False, lib=gpu_lib)
    assert ng.assert_matches_golden(name, ng.device_backend(mt)) >= 100
    mt.close()


def test_w_zero_and_dist_zero_at_header_level(gpu_lib):
    assert nc.check_header_level(gpu_lib) == [5, 11]


def test_error_returns_leave_records_and_mask_untouched(gpu_lib):
    nc.check_errors(gpu_lib)


def test_next_to_other_matcher_calls(gpu_lib):
    nc.check_threads(gpu_lib)


def test_stereo_parallax_cosine_device_equals_host(gpu_lib):
    """cos(2 * atan2(mb / 2, depth)): the device's fp64-routed divisions against the host's fp32 ones, bit for bit, on 2^16
    depths of [0.25, 512] m, and on 0, negative depths and infinity"""
    lib = gpu_lib
    lib.rgbl_test_np_cos_parallax.restype, lib.rgbl_test_np_cos_parallax.argtypes = C.c_float, [C.c_float, C.c_float]
    lib.rgbl_test_np_cos_parallax_device.restype = C.c_int
    lib.rgbl_test_np_cos_parallax_device.argtypes = [C.c_float, C.c_void_p, C.c_void_p, C.c_int]
    lo, hi = np.array([0.25, 512.0], np.float32).view(np.uint32)
    d = np.concatenate([np.linspace(int(lo), int(hi), 1 << 16).astype(np.uint32).view(np.float32),
                        np.array([0.0, -0.0, -1.0, -30.0, np.inf, 1e-30, 1e30], np.float32)])
    got = np.zeros(len(d), np.float32)
    for mb in (0.5372, 0.1, 1.1):
        assert lib.rgbl_test_np_cos_parallax_device(mb, d.ctypes.data, got.ctypes.data, len(d)) == 0
        want = np.array([lib.rgbl_test_np_cos_parallax(mb, float(x)) for x in d], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), d[got.view(np.uint32) != want.view(np.uint32)][:8]


def test_kitti_sized_key_frame(gpu_lib):
    """2 000 features, 10 neighbours, resident frames (what tools/new_points_bench.py times)"""
    assert nc.check_kitti_size(gpu_lib) > 300
