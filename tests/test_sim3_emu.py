"""rgbl_sim3_ransac - Sim3Solver (src/Sim3Solver.cc), every hypothesis of a call at once: the checks of tests/sim3_checks.py on
the CPU, with the kernel SOURCE of csrc/ransac.hip (k_sim3_hypotheses, k_sim3_select) running under the SIMT emulator of
tests/emu against the host build of csrc/sim3_math.h, bit for bit.  tests/test_sim3_gpu.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import sim3_checks as sk
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("n_hyp", sk.NHYPS)
@pytest.mark.parametrize("n", sk.NS)
def test_every_size_against_the_host_build(emu_lib, mt, n, n_hyp, fix_scale):
    sk.check_size(emu_lib, mt, n, n_hyp, fix_scale)


def test_pool_form_equals_host_arrays(emu_lib, mt):
    assert sk.check_pool(emu_lib, mt) > 0


def test_degenerate_samples(emu_lib, mt):
    sk.check_degenerate(emu_lib, mt)


def test_selection_rule(emu_lib, mt):
    sk.check_selection(emu_lib, mt)


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_single_calls(emu_lib, mt, B):
    assert sk.check_batch(emu_lib, mt, B) >= (1 if B == 1 else 2)


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    sk.check_errors(emu_lib, mt)


def test_next_to_other_matcher_calls(emu_lib):
    sk.check_threads(emu_lib)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib, frontend as F\n"
            "import sim3_checks as sk\n"
            "lib = _lib.bind(%r)\n"
            "mt = F.ORBmatcher(0.6, False, lib=lib)\n"
            "for n, h in ((65, 5), (257, 20), (1025, 3), (64, 300)): sk.check_size(lib, mt, n, h, 0)\n"
            "sk.check_batch(lib, mt, 3)\n"
            "sk.check_selection(lib, mt)\n"
            "print('sizes ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sizes ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
