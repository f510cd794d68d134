"""Device-side isInFrustum, the one-call SearchLocalPoints and the map-point pool on a real MI355X: the checks of
tests/local_map_checks.py on the product library (tests/test_local_map_emu.py runs them under the emulator), the device
build of logf_glibc against the live libm, and a local map of KITTI size."""
import ctypes as C

import numpy as np
import pytest

import local_map_checks as lc
import test_logf_glibc as tl
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu


def test_device_logf_equals_libm(gpu_lib):
    """k_test_logf: the restatement compiled for gfx950 (double arithmetic without contraction, fp32 denormals kept)."""
    rng = np.random.default_rng(2)
    with np.errstate(all="ignore"):
        xs = np.concatenate([tl.SPECIAL, (np.float32(1.2) ** np.arange(-9, 10)).astype(np.float32),
                             rng.integers(0x39800000, 0x45800000, 60000).astype(np.uint32).view(np.float32),    # [2^-12, 2^12]
                             rng.integers(0, 0x7f800000, 20000).astype(np.uint32).view(np.float32)])
    got = np.zeros(len(xs), np.float32)
    assert gpu_lib.rgbl_test_logf_device(xs.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), len(xs)) == 0
    m = tl.libm()
    want = np.array([m.logf(float(x)) for x in xs], np.float32)
    assert tl.same(got, want).all(), xs[~tl.same(got, want)][:16]


def test_cull_against_restatement_0_to_600_points(gpu_lib):
    assert lc.check_cull_sizes(gpu_lib) > 300


def test_fused_call_against_separate_calls_and_oracle(gpu_lib):
    lc.check_fused(gpu_lib)


def test_pool_form_equals_host_array_form(gpu_lib):
    lc.check_pool(gpu_lib)


def test_special_inputs(gpu_lib):
    lc.check_special(gpu_lib)


def test_error_returns(gpu_lib):
    lc.check_errors(gpu_lib)


def test_update_while_searching(gpu_lib):
    lc.check_threads(gpu_lib)


def test_kitti_sized_local_map(gpu_lib):
    """3 000 local map points against a 2 000-feature frame (what tools/local_map_bench.py times): host arrays and pool."""
    case = cases.make_local_map_case(3000, 2000, seed=41)
    mt = F.ORBmatcher(0.8, True, lib=gpu_lib)
    want = lc.expected_fused(case, 3.0, 0.8)
    assert want[2] > 1200 and want[4] > 300
    lc.assert_fused(mt.SearchLocalPoints(case, 3.0), want, "3000 points")
    pool, pc = lc.pooled(gpu_lib, case)
    lc.assert_fused(mt.SearchLocalPoints(pc, 3.0), want, "3000 pooled points")
    pool.close()
    mt.close()
