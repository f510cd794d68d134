"""rgbl_optimize_sim3 - Optimizer::OptimizeSim3 (Optimizer.cc:2115-2381) in one workgroup per candidate: the checks of
tests/sim3_opt_checks.py on the CPU, with the kernel SOURCE of csrc/optimize.hip (k_sim3_opt) running under the SIMT emulator of
tests/emu against the host build of csrc/sim3opt_math.h, bit for bit: estimate, flags, count, counters and diagnostics; and the
call's size limits from both sides.  tests/test_sim3_opt_gpu.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import sim3_opt_checks as oc
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("matched", oc.SIZES)
def test_every_size_against_the_host_build(emu_lib, mt, matched, fix_scale):
    oc.check_size(emu_lib, mt, matched, fix_scale)


def test_point_on_and_behind_the_camera_plane(emu_lib, mt):
    oc.check_degenerate_depth(emu_lib, mt)


def test_problems_without_any_edge(emu_lib, mt):
    oc.check_no_edge(emu_lib, mt)


@pytest.mark.parametrize("B", [1, 3, 300])
def test_batch_equals_single_calls(emu_lib, mt, B):
    assert (oc.check_batch(emu_lib, mt, B) > 0) == (B > 1)   # problem 0 has no feature at all


def test_resident_frames_and_pool_equal_host_arrays(emu_lib, mt):
    assert oc.check_resident(emu_lib, mt) > 150


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    oc.check_errors(emu_lib, mt)


def test_next_to_other_matcher_calls(emu_lib):
    oc.check_threads(emu_lib)


def test_exp_quotient_and_root_emulated_equal_host(emu_lib):
    assert oc.check_math_device(emu_lib) > 40000


def test_65535_features_in_both_key_frames(emu_lib, mt):
    assert oc.check_limit(emu_lib, mt) > 900


def test_65536_features_and_32768_problems_are_refused(emu_lib, mt):
    oc.check_limit_refused(emu_lib, mt)


def test_16_levels_accepted_17_refused(emu_lib, mt):
    oc.check_levels_limit(emu_lib, mt)


@pytest.mark.parametrize("order", ["desc", "shuffle"])
def test_kernel_is_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib, frontend as F\n"
            "import sim3_opt_checks as oc\n"
            "lib = _lib.bind(%r)\n"
            "mt = F.ORBmatcher(0.6, False, lib=lib)\n"
            "for n in (10, 257, 2049): oc.check_size(lib, mt, n, n == 257)\n"
            "oc.check_batch(lib, mt, 3)\n"
            "oc.check_degenerate_depth(lib, mt)\n"
            "print('sizes ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sizes ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
