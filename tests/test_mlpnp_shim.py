"""The C++ drop-in rgbl_shim::MLPnPsolver<Frame, MapPoint> (shim/MLPnPsolver.h): instantiated with the stand-in Frame, MapPoint
and camera the reference's own MLPnPsolver functions are compiled against (tests/mlpnp_ref_types.h), behind the glue that records
the reference's runs (tests/mlpnp_ref_glue.cpp, -DMLPNP_SHIM), and run on the cases of the fixtures under tests/golden/mlpnp.
Needs nothing of the reference: the inputs are regenerated from the fixtures' parameters, and the glue's DUtils::Random stand-in
over random_r must draw the very sets the reference's Random.cpp drew.  Checked per case, up to and including its first success
(after it the drop-in has drawn further than the reference: the documented deviation): the sets, the return values, bNoMore,
nInliers, mnIterations, mnBestInliers, the bits of Tout and of mBestTcw, and vbInliers.  The program itself checks IterateBatch
(two fresh solvers: the first gets the first recorded call; a batch over two devices is refused) and the two refusals (a camera
that is not a Pinhole, a minimal set other than six).  With the emulated kernels here, and on the MI355X."""
import os

import pytest

import mlpnp_golden as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_all(exe):
    n = 0
    for name in sorted(mg.CASES):
        n += mg.check_shim_against_fixture(mg.shim_run(exe, mg.CASES[name]), mg.load(name))
    return n


def test_drop_in_reproduces_the_fixtures_on_the_emulator(emu_lib):
    assert run_all(mg.build_shim(emu_lib._name, "emu")) == len(mg.CASES)


@pytest.mark.gpu
def test_drop_in_reproduces_the_fixtures_on_mi355x(gpu_lib):
    assert run_all(mg.build_shim(os.path.join(ROOT, "orb_slam3_rgbl_amd", "librgbl_frontend.so"), "gpu")) == len(mg.CASES)
