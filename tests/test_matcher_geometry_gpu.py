"""The grid-walking matcher searches beyond the KITTI camera and the (8, 1.2) pyramid on the hardware, against the oracle: the
matrix of tests/test_matcher_geometry_emu.py at the emulator tier's size and at one that crosses the kernels' LDS forms
(kGridLdsN2 = 8192 features; kResolveLdsN1 = 8192 points, kResolveLdsN2 = 6144 features), the points placed on the bounds, and
the EuRoC grid through resident frames.  The sizes at the library's limits - 65535 features, 2^20 - 1 points, one past each - are
in tests/test_limits_gpu.py and tests/test_limits_emu.py (cases: tests/limit_cases.py)."""
import pytest

import geometry_checks as gc
import parity_checks as pc

@pytest.mark.gpu
@pytest.mark.parametrize("camera,pyramid", gc.MATRIX, ids=gc.MATRIX_IDS)
@pytest.mark.parametrize("name", sorted(gc.SEARCHES))
def test_search_on_camera_and_pyramid(gpu_lib, name, camera, pyramid):
    gc.check_search(gpu_lib, name, camera, pyramid, 1200, 1000)
    gc.check_search(gpu_lib, name, camera, pyramid, *gc.beyond_lds(name))


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["cells_of_2x2_px", "euroc_undistorted"])
def test_points_on_the_bounds_and_features_on_the_window_edges(gpu_lib, grid):
    found = pc.check_grid_search_bounds(gpu_lib, pc.POW2_GRID if grid == "cells_of_2x2_px" else gc.camera(grid).grid())
    assert len(found) == len(pc.BOUNDS_SEARCHES)


@pytest.mark.gpu
def test_resident_frames_with_the_euroc_grid(gpu_lib):
    gc.check_resident_frames(gpu_lib)
    gc.check_resident_frames(gpu_lib, "small_offset", (16, 1.1), 1200, 8300)


@pytest.mark.gpu
def test_seventeen_levels_are_refused_by_every_grid_search_entry_point(gpu_lib):
    gc.check_seventeen_levels_refused(gpu_lib)
