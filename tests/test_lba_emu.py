"""rgbl_local_bundle_adjustment - Optimizer::LocalBundleAdjustment (Optimizer.cc:1188-1497) as one problem spread over the
device: the checks of tests/lba_checks.py on the CPU, with the kernel SOURCE of csrc/lba.hip running under the SIMT emulator of
tests/emu against the host build of csrc/lba_math.h, bit for bit in every output byte, the NaN and failed-factorisation paths
included.  tests/test_lba_gpu.py runs the same checks on the MI355X."""
import pytest

import lba_checks as lk
from orb_slam3_rgbl_amd import frontend as F


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("name", lk.DIRECTED)
def test_directed_case_equals_the_host_build(emu_lib, mt, name):
    lk.check_directed(emu_lib, mt, name)


@pytest.mark.parametrize("n", lk.LANE_SIZES)
def test_sizes_around_every_lane_count(emu_lib, mt, n):
    lk.check_lane_size(emu_lib, mt, n)


def test_stop_flag_at_entry_and_at_every_poll(emu_lib, mt):
    assert lk.check_stop(emu_lib, mt) > 12


def test_pool_form_equals_host_arrays_and_stays_untouched_without_a_run(emu_lib, mt):
    lk.check_pool(emu_lib, mt)


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    lk.check_errors(emu_lib, mt)
