"""rgbl_local_bundle_adjustment on a real MI355X: the checks of tests/lba_checks.py on the product library against ITS host build
of csrc/lba_math.h, bit for bit in every output byte (tests/test_lba_emu.py runs them under the emulator), and every size limit
from both sides."""
import pytest

import lba_checks as lk
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("name", lk.DIRECTED)
def test_directed_case_equals_the_host_build(gpu_lib, mt, name):
    lk.check_directed(gpu_lib, mt, name)


@pytest.mark.parametrize("n", lk.LANE_SIZES)
def test_sizes_around_every_lane_count(gpu_lib, mt, n):
    lk.check_lane_size(gpu_lib, mt, n)


def test_stop_flag_at_entry_and_at_every_poll(gpu_lib, mt):
    assert lk.check_stop(gpu_lib, mt) > 12


def test_pool_form_equals_host_arrays_and_stays_untouched_without_a_run(gpu_lib, mt):
    lk.check_pool(gpu_lib, mt)


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    lk.check_errors(gpu_lib, mt)


def test_every_limit_from_both_sides(gpu_lib, mt):
    lk.check_limits(gpu_lib, mt)
