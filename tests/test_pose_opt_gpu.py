"""rgbl_pose_optimization on a real MI355X: the checks of tests/pose_opt_checks.py on the product library against ITS host
build of csrc/poseopt_math.h, bit for bit (tests/test_pose_opt_emu.py runs them under the emulator), the header's sin / cos,
quotient and square root device against host, and the float64 model at n = 300 within the recorded tolerance."""
import json
import os

import numpy as np
import pytest

import pose_opt_checks as pc
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_opt")


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("kind", list(pc.KINDS))
@pytest.mark.parametrize("matched", pc.SIZES)
def test_every_size_against_the_host_build(gpu_lib, mt, matched, kind):
    pc.check_size(gpu_lib, mt, matched, kind)


def test_every_size_gives_the_recorded_bits(mt):
    """the device against tests/golden/pose_opt/host_bits.json (what the host build gave when it was recorded), not against the
    host build next to it: a change that moves both together fails here"""
    import host_bits as hb
    want = hb.recorded("pose_opt")
    for name, case, _ in hb.pose_size_cases():
        assert hb.pose_record(mt.PoseOptimization(case, outlier_fill=hb.FILL)) == want[name], name


def test_every_correspondence_an_outlier_after_round_0(gpu_lib, mt):
    pc.check_all_outliers(gpu_lib, mt)


def test_point_at_and_behind_the_camera_plane(gpu_lib, mt):
    pc.check_degenerate_depth(gpu_lib, mt)


@pytest.mark.parametrize("B", [1, 3, 300])
def test_batch_equals_single_calls(gpu_lib, mt, B):
    assert (pc.check_batch(gpu_lib, mt, B) > 0) == (B > 1)   # problem 0 has no feature at all


def test_resident_frame_and_pool_equal_host_arrays(gpu_lib, mt):
    assert pc.check_resident(gpu_lib, mt) > 200


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    pc.check_errors(gpu_lib, mt)


def test_next_to_other_matcher_calls(gpu_lib):
    pc.check_threads(gpu_lib)


def test_sin_cos_quotient_and_root_device_equal_host(gpu_lib):
    assert pc.check_math_device(gpu_lib) > 40000


def test_against_the_float64_model(gpu_lib, mt):
    """n = 300, the motion-model case: pose within the recorded tolerance (100 x the model's own reordering noise,
    tests/golden/pose_opt/README.md), flags and count equal"""
    import pose_opt_model as pm
    tol = json.load(open(os.path.join(GOLDEN, "tolerance.json")))["tolerance"]
    case = cases.make_pose_opt_case(2000, 300, seed=3)
    want = pm.run(case)
    assert want["margin"] > 1e-6
    got = mt.PoseOptimization(case)
    R = pm.quat_to_rot(got["q64"])
    err = max(np.abs(R - want["R"]).max(), np.abs(got["t64"] - want["t"]).max())
    print("pose difference to the model %.3g (tolerance %.3g)" % (err, tol))
    assert err <= tol
    assert np.array_equal(got["outlier"], want["outlier"]) and got["result"] == want["result"]
    assert np.array_equal(got["iterations"], want["iterations"]) and np.array_equal(got["active"], want["active"])
