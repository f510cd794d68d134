"""rgbl_optimize_sim3 on a real MI355X: the checks of tests/sim3_opt_checks.py on the product library against ITS host build of
csrc/sim3opt_math.h, bit for bit (tests/test_sim3_opt_emu.py runs them under the emulator), the header's exp, quotient and
square root device against host, and the float64 model at (2000, 300) within the recorded tolerance."""
import json
import os

import numpy as np
import pytest

import sim3_opt_checks as oc
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import sim3_cases as sc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_opt")


@pytest.fixture(scope="module")
def mt(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    yield m
    m.close()


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("matched", oc.SIZES)
def test_every_size_against_the_host_build(gpu_lib, mt, matched, fix_scale):
    oc.check_size(gpu_lib, mt, matched, fix_scale)


def test_every_size_gives_the_recorded_bits(mt):
    """the device against tests/golden/sim3_opt/host_bits.json (what the host build gave when it was recorded), not against the
    host build next to it: a change that moves both together fails here"""
    import host_bits as hb
    want = hb.recorded("sim3_opt")
    for name, case, _ in hb.sim3_size_cases():
        assert hb.sim3_record(mt.OptimizeSim3(case, cleared_fill=hb.FILL)) == want[name], name


def test_point_on_and_behind_the_camera_plane(gpu_lib, mt):
    oc.check_degenerate_depth(gpu_lib, mt)


def test_problems_without_any_edge(gpu_lib, mt):
    oc.check_no_edge(gpu_lib, mt)


@pytest.mark.parametrize("B", [1, 3, 300])
def test_batch_equals_single_calls(gpu_lib, mt, B):
    assert (oc.check_batch(gpu_lib, mt, B) > 0) == (B > 1)   # problem 0 has no feature at all


def test_resident_frames_and_pool_equal_host_arrays(gpu_lib, mt):
    assert oc.check_resident(gpu_lib, mt) > 150


def test_error_returns_leave_the_outputs_untouched(gpu_lib, mt):
    oc.check_errors(gpu_lib, mt)


def test_limits_from_both_sides(gpu_lib, mt):
    assert oc.check_limit(gpu_lib, mt) > 900
    oc.check_limit_refused(gpu_lib, mt)
    oc.check_levels_limit(gpu_lib, mt)


def test_next_to_other_matcher_calls(gpu_lib):
    oc.check_threads(gpu_lib)


def test_exp_quotient_and_root_device_equal_host(gpu_lib):
    assert oc.check_math_device(gpu_lib) > 40000


def test_against_the_float64_model(gpu_lib, mt):
    """(2000, 300), both fix_scale values: the estimate within the recorded tolerance (16 x the model's own reordering noise,
    tests/golden/sim3_opt/README.md), flags, counters and iterations equal.  Measured on the MI355X: 9.1e-9 and 5.1e-9, the
    host build's own differences."""
    import sim3_opt_model as sm
    rec = json.load(open(os.path.join(GOLDEN, "tolerance.json")))
    for fix_scale in (False, True):
        case = sc.make_sim3_opt_case(2000, 300, seed=4, fix_scale=fix_scale)
        with np.errstate(all="ignore"):
            want = sm.run(case)
        assert want["margin"] > rec["chi2_margin"]
        got = mt.OptimizeSim3(case, cleared_fill=2)
        err = sm.difference(dict(R=sm.quat_to_rot(got["q"]), t=got["t"], s=got["s"]), want)
        print("fix_scale %d: estimate difference to the model %.3g (tolerance %.3g)" % (fix_scale, err, rec["tolerance"]))
        assert err <= rec["tolerance"]
        assert np.array_equal(got["cleared"], want["cleared"]) and got["result"] == want["result"] and got["n_bad"] == want["n_bad"]
        assert np.array_equal(got["iterations"], want["iterations"]) and np.array_equal(got["active"], want["active"])
        for k in ("n_correspondences", "n_bad_mps", "n_in_kf2", "n_out_kf2", "n_without_mp"):
            assert got[k] == want[k], k
