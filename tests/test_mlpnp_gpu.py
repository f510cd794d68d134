"""rgbl_mlpnp_ransac on a real MI355X: the checks of tests/mlpnp_checks.py on the product library against ITS host build of
csrc/mlpnp_math.h, bit for bit (tests/test_mlpnp_emu.py runs them under the emulator), and the float64 model at N = 100 within the
recorded tolerance."""
import pytest

import mlpnp_checks as mk
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("n_hyp", mk.NHYPS)
@pytest.mark.parametrize("N", mk.NS)
def test_every_size_against_the_host_build(gpu_lib, mt, N, n_hyp):
    mk.check_size(gpu_lib, mt, N, n_hyp)


def test_pool_and_resident_frame_equal_host_arrays(gpu_lib, mt):
    assert mk.check_forms(gpu_lib, mt) > 0


def test_planar_scenes(gpu_lib, mt):
    assert mk.check_planar(gpu_lib, mt) >= 1


def test_degenerate_samples(gpu_lib, mt):
    mk.check_degenerate(gpu_lib, mt)


def test_stop_rule(gpu_lib, mt):
    assert len(mk.check_scan(gpu_lib, mt)) == 9


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_single_calls(gpu_lib, mt, B):
    assert mk.check_batch(gpu_lib, mt, B) >= (1 if B == 1 else 2)


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    mk.check_errors(gpu_lib, mt)


def test_every_size_limit_from_both_sides(gpu_lib, mt):
    mk.check_limits(gpu_lib, mt)


def test_most_correspondences(gpu_lib, mt):
    assert mk.check_limit_n(gpu_lib, mt) <= mk.N_MAX


def test_most_hypotheses(gpu_lib, mt):
    assert mk.check_limit_hyp(gpu_lib, mt) >= 0


def test_next_to_other_matcher_calls(gpu_lib):
    mk.check_threads(gpu_lib)


def test_against_the_float64_model(gpu_lib, mt):
    """N = 100, 300 hypotheses: every compared hypothesis within the recorded tolerance (16 x the model's own reordering noise,
    tests/golden/mlpnp/README.md), the flags of every decided pair equal, the stop equal"""
    import test_mlpnp_math as tm
    pr, fwd, _ = tm.prepared(tm.GPU_CASE)
    assert fwd["N"] == 100
    tm.compare(mt.MLPnPRansac(pr), fwd, tm.load_recorded(), "MI355X, case %s" % (tm.CASES[tm.GPU_CASE],), tm.all_flags(mt, pr, host=False))
