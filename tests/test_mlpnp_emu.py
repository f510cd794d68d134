"""rgbl_mlpnp_ransac - MLPnPsolver (src/MLPnPsolver.cpp), every hypothesis of a call at once: the checks of tests/mlpnp_checks.py on
the CPU, with the kernel SOURCE of csrc/ransac.hip (k_mlpnp_hypotheses, k_mlpnp_select) running under the SIMT emulator of
tests/emu against the host build of csrc/mlpnp_math.h, bit for bit.  tests/test_mlpnp_gpu.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import mlpnp_checks as mk
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("n_hyp", mk.NHYPS)
@pytest.mark.parametrize("N", mk.NS)
def test_every_size_against_the_host_build(emu_lib, mt, N, n_hyp):
    mk.check_size(emu_lib, mt, N, n_hyp)


def test_pool_and_resident_frame_equal_host_arrays(emu_lib, mt):
    assert mk.check_forms(emu_lib, mt) > 0


def test_planar_scenes(emu_lib, mt):
    assert mk.check_planar(emu_lib, mt) >= 1


def test_degenerate_samples(emu_lib, mt):
    mk.check_degenerate(emu_lib, mt)


def test_stop_rule(emu_lib, mt):
    assert len(mk.check_scan(emu_lib, mt)) == 9


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_single_calls(emu_lib, mt, B):
    assert mk.check_batch(emu_lib, mt, B) >= (1 if B == 1 else 2)


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    mk.check_errors(emu_lib, mt)


def test_every_size_limit_from_both_sides(emu_lib, mt):
    mk.check_limits(emu_lib, mt)


def test_most_correspondences(emu_lib, mt):
    assert mk.check_limit_n(emu_lib, mt) <= mk.N_MAX


def test_next_to_other_matcher_calls(emu_lib):
    mk.check_threads(emu_lib, rounds=2)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib, frontend as F\n"
            "import mlpnp_checks as mk\n"
            "lib = _lib.bind(%r)\n"
            "mt = F.ORBmatcher(0.6, False, lib=lib)\n"
            "for N, h in ((65, 5), (257, 20), (300, 3)): mk.check_size(lib, mt, N, h)\n"
            "mk.check_planar(lib, mt)\n"
            "print('sizes ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sizes ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
