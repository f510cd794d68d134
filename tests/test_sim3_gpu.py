"""rgbl_sim3_ransac on a real MI355X: the checks of tests/sim3_checks.py on the product library against ITS host build of
csrc/sim3_math.h, bit for bit (tests/test_sim3_emu.py runs them under the emulator), and the float64 model at n = 100 within the
recorded tolerance."""
import numpy as np
import pytest

import sim3_checks as sk
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("fix_scale", [0, 1])
@pytest.mark.parametrize("n_hyp", sk.NHYPS)
@pytest.mark.parametrize("n", sk.NS)
def test_every_size_against_the_host_build(gpu_lib, mt, n, n_hyp, fix_scale):
    sk.check_size(gpu_lib, mt, n, n_hyp, fix_scale)


def test_pool_form_equals_host_arrays(gpu_lib, mt):
    assert sk.check_pool(gpu_lib, mt) > 0


def test_degenerate_samples(gpu_lib, mt):
    sk.check_degenerate(gpu_lib, mt)


def test_selection_rule(gpu_lib, mt):
    sk.check_selection(gpu_lib, mt)


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_single_calls(gpu_lib, mt, B):
    assert sk.check_batch(gpu_lib, mt, B) >= (1 if B == 1 else 2)


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    sk.check_errors(gpu_lib, mt)


def test_next_to_other_matcher_calls(gpu_lib):
    sk.check_threads(gpu_lib)


def test_against_the_float64_model(gpu_lib, mt):
    """n = 100, 300 hypotheses: every compared hypothesis within the recorded tolerance (16 x the model's own float32 / float64
    difference, tests/golden/sim3/README.md), the flags of every decided pair equal, the selection equal"""
    import json
    import os

    import sim3_model as sm
    import test_sim3_math as tm
    recorded = json.load(open(os.path.join(tm.GOLDEN, "tolerance.json")))
    pr = tm.make(tm.GPU_CASE)
    assert len(pr["max_err1"]) == 100
    m64 = sm.run(pr, np.float64)
    tm.compare(mt.Sim3Ransac(pr), m64, recorded, "MI355X, case %s" % (tm.CASES[tm.GPU_CASE],), tm.all_flags(mt, pr, host=False))
