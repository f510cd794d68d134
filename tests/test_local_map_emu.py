"""Device-side isInFrustum and the one-call SearchLocalPoints: the checks of tests/local_map_checks.py on the CPU, with the
kernel SOURCES of csrc/matcher.hip (k_frustum, k_map_points_scatter and the search kernels behind them) running under the
SIMT emulator of tests/emu.  tests/test_local_map_gpu.py runs the same checks on the MI355X."""
import os
import subprocess
import sys

import pytest

import local_map_checks as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cull_against_restatement_0_to_600_points(emu_lib):
    assert lc.check_cull_sizes(emu_lib) > 300


def test_fused_call_against_separate_calls_and_oracle(emu_lib):
    lc.check_fused(emu_lib)


def test_pool_form_equals_host_array_form(emu_lib):
    lc.check_pool(emu_lib)


def test_special_inputs(emu_lib):
    lc.check_special(emu_lib)


def test_error_returns(emu_lib):
    lc.check_errors(emu_lib)


def test_update_while_searching(emu_lib):
    lc.check_threads(emu_lib)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib\n"
            "import local_map_checks as lc\n"
            "lib = _lib.bind(%r)\n"
            "print('seen', lc.check_cull_sizes(lib, sizes=(65, 600)))\n"
            "print('matched', lc.check_fused(lib))\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "matched" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
