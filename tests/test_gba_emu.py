"""rgbl_bundle_adjustment - Optimizer::BundleAdjustment (Optimizer.cc:52-390), the global bundle adjustment with its panel
LDL^T across the device: the checks of tests/gba_checks.py on the CPU, with the kernel SOURCE of csrc/gba.hip and csrc/lba.hip
running under the SIMT emulator of tests/emu against the host build (csrc/lba_math.h with lm_solve_panel), bit for bit in every
output byte.  tests/test_gba_gpu.py runs the same checks on the MI355X."""
import pytest

import gba_checks as gk
from orb_slam3_rgbl_amd import frontend as F


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("name", gk.DIRECTED)
def test_directed_case_equals_the_host_build(emu_lib, mt, name):
    gk.check_directed(emu_lib, mt, name)


def test_stop_flag_at_entry_and_at_every_poll(emu_lib, mt):
    assert gk.check_stop(emu_lib, mt) > 6


def test_pool_form_equals_host_arrays_and_errors_leave_the_pool_untouched(emu_lib, mt):
    gk.check_pool(emu_lib, mt)


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    gk.check_errors(emu_lib, mt)
