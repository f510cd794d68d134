"""rgbl_bundle_adjustment on a real MI355X: the checks of tests/gba_checks.py on the product library against ITS host build,
bit for bit in every output byte (tests/test_gba_emu.py runs them under the emulator), and one case of 256 active cameras
(n = 1 536, 48 panels) that the emulator tier leaves out."""
import pytest

import gba_checks as gk
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("name", gk.DIRECTED)
def test_directed_case_equals_the_host_build(gpu_lib, mt, name):
    gk.check_directed(gpu_lib, mt, name)


def test_256_active_cameras_equal_the_host_build(gpu_lib, mt):
    h = gk.both(gpu_lib, mt, gk.sized(256, n_points=1200, max_iterations=1), "256 active cameras")
    assert h["active_cams"] == 256 and h["failed"] == 0 and h["iterations"] == 1 and h["last_chi2"] < h["first_chi2"]


def test_stop_flag_at_entry_and_at_every_poll(gpu_lib, mt):
    assert gk.check_stop(gpu_lib, mt) > 6


def test_pool_form_equals_host_arrays_and_errors_leave_the_pool_untouched(gpu_lib, mt):
    gk.check_pool(gpu_lib, mt)


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    gk.check_errors(gpu_lib, mt)
