"""rgbl_pose_optimization - Optimizer::PoseOptimization (Optimizer.cc:814-1114) in one workgroup per frame: the checks of
tests/pose_opt_checks.py on the CPU, with the kernel SOURCE of csrc/optimize.hip (k_pose_opt) running under the SIMT emulator of
tests/emu against the host build of csrc/poseopt_math.h, bit for bit: pose, flags, count and diagnostics.
tests/test_pose_opt_gpu.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import pose_opt_checks as pc
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("kind", list(pc.KINDS))
@pytest.mark.parametrize("matched", pc.SIZES)
def test_every_size_against_the_host_build(emu_lib, mt, matched, kind):
    pc.check_size(emu_lib, mt, matched, kind)


def test_every_correspondence_an_outlier_after_round_0(emu_lib, mt):
    pc.check_all_outliers(emu_lib, mt)


def test_point_at_and_behind_the_camera_plane(emu_lib, mt):
    pc.check_degenerate_depth(emu_lib, mt)


@pytest.mark.parametrize("B", [1, 3, 300])
def test_batch_equals_single_calls(emu_lib, mt, B):
    assert (pc.check_batch(emu_lib, mt, B) > 0) == (B > 1)   # problem 0 has no feature at all


def test_resident_frame_and_pool_equal_host_arrays(emu_lib, mt):
    assert pc.check_resident(emu_lib, mt) > 200


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    pc.check_errors(emu_lib, mt)


def test_next_to_other_matcher_calls(emu_lib):
    pc.check_threads(emu_lib)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernel_is_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib, frontend as F\n"
            "import pose_opt_checks as pc\n"
            "lib = _lib.bind(%r)\n"
            "mt = F.ORBmatcher(0.6, False, lib=lib)\n"
            "for n in (10, 257, 2049): pc.check_size(lib, mt, n, 'mixed')\n"
            "pc.check_batch(lib, mt, 3)\n"
            "print('sizes ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sizes ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
