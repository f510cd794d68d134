"""rgbl_map_points_refresh - MapPoint::UpdateNormalAndDepth and ComputeDistinctiveDescriptors for pool slots, from observations
in device-resident key frames: the checks of tests/map_refresh_checks.py on the CPU, with the kernel SOURCES of csrc/matcher.hip
(k_map_refresh_normal, k_map_refresh_desc) running under the SIMT emulator of tests/emu.  tests/test_map_refresh_gpu.py runs
the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import map_refresh_checks as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_kfs", mr.KF_COUNTS)
def test_every_size_against_restatement_and_oracle(emu_lib, n_kfs):
    assert mr.check_sizes(emu_lib, n_kfs) == sum(mr.POINT_COUNTS) * sum(mr.OBS_COUNTS)


def test_rules_of_the_two_reference_functions(emu_lib):
    mr.check_rules(emu_lib)


def test_wide_range_of_magnitudes_and_a_point_on_a_camera_centre(emu_lib):
    mr.check_wide_range(emu_lib)


def test_track_local_points_on_the_refreshed_pool(emu_lib):
    assert mr.check_track_after_refresh(emu_lib) > 10


def test_error_returns_leave_the_pool_unchanged(emu_lib):
    mr.check_errors(emu_lib)


def test_refresh_next_to_search_and_update(emu_lib):
    mr.check_threads(emu_lib)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib\n"
            "import map_refresh_checks as mr\n"
            "lib = _lib.bind(%r)\n"
            "print('pairs', mr.check_sizes(lib, 2, points=(65,)))\n"
            "mr.check_rules(lib)\n"
            "print('rules ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "rules ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
