"""rgbl_create_new_map_points / rgbl_triangulate_matches - LocalMapping::CreateNewMapPoints from its neighbour loop on, one call:
the checks of tests/new_points_checks.py on the CPU, with the kernel SOURCES of csrc/matcher.hip (k_search_triangulation,
k_new_points) running under the SIMT emulator of tests/emu.  tests/test_new_points_gpu.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import new_points_checks as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_neigh", nc.NEIGHBOUR_COUNTS)
def test_every_size_against_the_restatement(emu_lib, n_neigh):
    total = nc.check_sizes(emu_lib, n_neigh)
    assert (total > 100) == (n_neigh > 0)


def test_main_fixture_chain_and_status_coverage(emu_lib):
    counts = nc.check_main(emu_lib)
    assert all(counts[s] >= 3 for s in nc.STATUSES_IN_FIXTURE)


def test_more_matches_than_one_tile_in_one_launch(emu_lib):
    assert nc.check_dense(emu_lib) > 512


def test_w_zero_and_dist_zero_at_header_level(emu_lib):
    assert nc.check_header_level(emu_lib) == [5, 11]


def test_error_returns_leave_records_and_mask_untouched(emu_lib):
    nc.check_errors(emu_lib)


def test_next_to_other_matcher_calls(emu_lib):
    nc.check_threads(emu_lib)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib\n"
            "import new_points_checks as nc\n"
            "lib = _lib.bind(%r)\n"
            "print('records', nc.check_sizes(lib, 10, sizes=(65, 257, 600)))\n"
            "nc.check_main(lib)\n"
            "print('main ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "main ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
