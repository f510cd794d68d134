"""rgbl_two_view_reconstruct on a real MI355X: the checks of tests/twoview_checks.py on the product library against ITS host build
of csrc/twoview_math.h, bit for bit (tests/test_twoview_emu.py runs them under the emulator), and the float64 model at N = 100 within the
recorded tolerance."""
import pytest

import twoview_checks as tk
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("n_hyp", tk.NHYPS)
@pytest.mark.parametrize("N", tk.NS)
def test_every_size_against_the_host_build(gpu_lib, mt, N, n_hyp):
    tk.check_size(gpu_lib, mt, N, n_hyp)


def test_every_scene_and_every_exit(gpu_lib, mt):
    taken = tk.check_scenes(gpu_lib, mt)
    assert set(taken) == {(1, tk.FOUND), (0, tk.FOUND), (-1, tk.NO_SCORE), (0, tk.H_RATIO), (0, tk.H_RULE), (1, tk.F_FEW_OR_SIMILAR), (1, tk.F_PARALLAX)}


def test_degenerate_sets(gpu_lib, mt):
    tk.check_degenerate(gpu_lib, mt)


def test_ties(gpu_lib, mt):
    tk.check_ties(gpu_lib, mt)


def test_resident_frames_equal_host_arrays(gpu_lib, mt):
    assert tk.check_forms(gpu_lib, mt) > 0


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_single_calls(gpu_lib, mt, B):
    assert tk.check_batch(gpu_lib, mt, B) >= (1 if B == 1 else 2)


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    tk.check_errors(gpu_lib, mt)


def test_every_size_limit_from_both_sides(gpu_lib, mt):
    tk.check_limits(gpu_lib, mt)


def test_most_matches(gpu_lib, mt):
    assert tk.check_limit_n(gpu_lib, mt) <= tk.N_MAX


def test_most_hypotheses(gpu_lib, mt):
    assert tk.check_limit_hyp(gpu_lib, mt) >= 0


def test_next_to_other_matcher_calls(gpu_lib):
    tk.check_threads(gpu_lib)


def test_against_the_float64_model(gpu_lib, mt):
    """a general scene, N = 100, 200 sets: every compared hypothesis within the recorded tolerance (16 x the model's own float32 /
    float64 difference, tests/golden/two_view/README.md), the winners, the choice, n_good and T21 as the model's"""
    import test_twoview_math as tm
    assert tm.CASES[tm.GPU_CASE][:2] == ("general", 100)
    worst, decided = tm.compare(mt.TwoViewReconstruct(tm.case_problem(tm.GPU_CASE)), tm.GPU_CASE, tm.load_recorded(), "MI355X, case %s" % tm.GPU_CASE)
    assert decided
