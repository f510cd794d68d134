"""The grid-walking matcher searches beyond the KITTI camera and the (8, 1.2) pyramid, kernel sources under the SIMT emulator
against the oracle (tests/geometry_checks.py holds the table of searches, cameras and pyramids)."""
import pytest

import geometry_checks as gc
import parity_checks as pc

SEARCH_NAMES = sorted(gc.SEARCHES)
# k_proj_grid<false> (frames beyond kGridLdsN2 = 8192 features) behind the best-only searches
BEYOND_GRID_LDS = ["fuse", "project_search_form0", "project_search_form1", "projection_sim3_form0", "projection_sim3_form2"]


@pytest.mark.parametrize("camera,pyramid", gc.MATRIX, ids=gc.MATRIX_IDS)
@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_every_case_clears_the_floor_with_the_oracle_alone(oracle, name, camera, pyramid):
    """no kernel involved: the cases the other tiers run are not empty (sizes of the emulator and the GPU tier)"""
    for n1, n2 in ((1200, 1000), gc.beyond_lds(name), (300, 8300)):
        gc.check_search(None, name, camera, pyramid, n1, n2)


def test_the_fixed_random_seeds_clear_the_floor_with_the_oracle_alone(oracle):
    import numpy as np

    import fuzz_cases
    import test_fuzz_gpu
    for kind in ("point_search", "greedy_search"):
        for seed in test_fuzz_gpu.SEEDS[kind]:
            rng = np.random.default_rng(seed)
            for _ in range(test_fuzz_gpu.PER_SEED[kind]):
                fuzz_cases.CASES[kind](None, rng)


@pytest.mark.parametrize("camera,pyramid", gc.MATRIX, ids=gc.MATRIX_IDS)
@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_search_on_camera_and_pyramid(emu_lib, name, camera, pyramid):
    gc.check_search(emu_lib, name, camera, pyramid, 1200, 1000)


@pytest.mark.parametrize("name", BEYOND_GRID_LDS)
def test_best_only_searches_beyond_the_grid_kernels_lds_form(emu_lib, name):
    gc.check_search(emu_lib, name, "small_offset", (16, 1.1), 300, 8300)
    gc.check_search(emu_lib, name, "euroc_undistorted", (12, 1.2), 300, 8300)


def test_seventeen_levels_are_refused_by_every_grid_search_entry_point(emu_lib):
    gc.check_seventeen_levels_refused(emu_lib)


@pytest.mark.parametrize("grid", ["cells_of_2x2_px", "euroc_undistorted"])
def test_points_on_the_bounds_and_features_on_the_window_edges(emu_lib, grid):
    found = pc.check_grid_search_bounds(emu_lib, pc.POW2_GRID if grid == "cells_of_2x2_px" else gc.camera(grid).grid())
    assert len(found) == len(pc.BOUNDS_SEARCHES)


def test_resident_frames_with_the_euroc_grid(emu_lib):
    gc.check_resident_frames(emu_lib)
