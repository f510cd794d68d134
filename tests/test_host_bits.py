"""The host builds of csrc/poseopt_math.h and csrc/sim3opt_math.h (rgbl_pose_optimization_host, rgbl_optimize_sim3_host) against
the bits recorded in tests/golden/*/host_bits.json, on every recorded case, and the kernel SOURCE under the SIMT emulator
against them on the cases with at most 257 correspondences (tests/test_*_opt_emu.py cover 2049 against the host build).
tests/host_bits.py says what a record holds."""
import pytest

import host_bits as hb
from orb_slam3_rgbl_amd import frontend as F

POSE = {name: (case, m) for name, case, m in hb.pose_cases()}
SIM3 = {name: (case, m) for name, case, m in hb.sim3_cases()}


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


def test_every_case_is_recorded():
    assert set(hb.recorded("pose_opt")) == set(POSE) and len(POSE) == 27 + 1 + 2 + 17
    assert set(hb.recorded("sim3_opt")) == set(SIM3) and len(SIM3) == 18 + 1 + 4 + 11


@pytest.mark.parametrize("name", list(POSE))
def test_pose_optimization_gives_the_recorded_bits(emu_lib, mt, name):
    case, m = POSE[name]
    want = hb.recorded("pose_opt")[name]
    assert hb.pose_record(F.pose_optimization_host(case, emu_lib, outlier_fill=hb.FILL)) == want, "host build"
    if m <= hb.EMU_MAX:
        assert hb.pose_record(mt.PoseOptimization(case, outlier_fill=hb.FILL)) == want, "emulated kernel"


@pytest.mark.parametrize("name", list(SIM3))
def test_optimize_sim3_gives_the_recorded_bits(emu_lib, mt, name):
    case, m = SIM3[name]
    want = hb.recorded("sim3_opt")[name]
    assert hb.sim3_record(F.optimize_sim3_host(case, emu_lib, cleared_fill=hb.FILL)) == want, "host build"
    if m <= hb.EMU_MAX:
        assert hb.sim3_record(mt.OptimizeSim3(case, cleared_fill=hb.FILL)) == want, "emulated kernel"
