"""Frame::isInFrustum + MapPoint::PredictScale: the restatement (F.frustum_restatement) and the emulated kernel against the
fixtures under tests/golden/frustum that the reference's own functions produced, those functions - cut out of the reference's
sources and compiled unmodified (tests/frustum_golden.py) - against the fixtures and against the restatement on fresh seeds, and
the one-call SearchLocalPoints against the chain reference isInFrustum -> reference ORBmatcher::SearchByProjection."""
import numpy as np
import pytest

import frustum_golden as fg
import local_map_checks as lc
from oracle import oracle_py as O
from oracle import ref_py as R
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

needs_reference = pytest.mark.skipif(not fg.have_reference(), reason="the reference sources are not on this machine")


@pytest.mark.parametrize("name", sorted(fg.CASES))
def test_restatement_matches_golden(name):
    assert fg.assert_matches_golden(name, fg.restatement_results) > 70


@pytest.mark.parametrize("name", sorted(fg.CASES))
def test_emulated_kernel_matches_golden(emu_lib, name):
    assert fg.assert_matches_golden(name, fg.device_results(emu_lib)) > 70


@pytest.mark.parametrize("name", sorted(fg.CASES))
def test_fixture_conditions(name):
    """Every exit of isInFrustum, every level, both clamps and the edge points, on the recorded results."""
    case, named, pick = fg.make_case(name)
    want = fg.load(name)["results"]
    iv, rec, _ = F.frustum_restatement(case)
    assert fg.encode(iv, rec, pick) == want           # ... so the conditions below are conditions on the recorded results
    fg.check_conditions(case, named, pick, iv, rec)
    assert len(pick) <= fg.MAX_POINTS


@needs_reference
@pytest.mark.parametrize("name", sorted(fg.CASES))
def test_reference_code_reproduces_golden(name):
    """The committed fixtures are what src/Frame.cc:602-664 + src/MapPoint.cc:531-546, compiled unmodified, leave in a MapPoint."""
    lib = fg.build_reference_glue()
    fg.assert_matches_golden(name, lambda case: fg.reference_results(case, lib))
    case, named, pick = fg.make_case(name)
    fg.check_conditions(case, named, pick, *fg.reference_results(case, lib))


@needs_reference
def test_restatement_equals_reference_code_on_fresh_seeds():
    lib = fg.build_reference_glue()
    n = 0
    for params in (dict(n1=900, n2=50, seed=7), dict(n1=450, n2=50, seed=8), dict(n1=2000, n2=50, seed=9)):
        case, _, _ = fg.make_case(**params)
        for variant in (case, dict(case, consider1=None), dict(case, n_levels=5), dict(case, viewing_cos_limit=np.float32(0.8))):
            iv, rec = fg.reference_results(variant, lib)
            lc.assert_cull((iv, rec, int(iv.sum())), F.frustum_restatement(variant), "seed %d" % params["seed"])
            n += int(iv.sum())
    assert n > 3000


@needs_reference
def test_fused_call_equals_the_reference_chain(emu_lib):
    """rgbl_track_local_points against the reference's isInFrustum followed by the reference's SearchByProjection(F,
    vpMapPoints, th, bFarPoints, thFarPoints) (oracle/_ref through oracle/ref_py.py)."""
    ref = R.load_matcher()
    if ref is None:
        pytest.skip("oracle/_ref is not built")
    lib = fg.build_reference_glue()
    mt = F.ORBmatcher(0.8, True, lib=emu_lib)
    for far in (0, 1):
        case = dict(fg.make_case("kitti")[0], far_points=far)
        iv, rec = fg.reference_results(case, lib)
        keep = []
        P = O.make_local_points_input(cases.local_points_from_cull(case, iv, rec), 3.0, 0.8, keep)
        m, nm, _ = R.call_struct(ref, "ref_search_local_points", P, P.n2)
        lc.assert_fused(mt.SearchLocalPoints(case, 3.0), (iv, rec, int(iv.sum()), m, nm), "reference chain, bFarPoints %d" % far)
        assert nm > 30   # a real search: with bFarPoints roughly half of the points in view are left
    mt.close()
