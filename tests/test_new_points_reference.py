"""LocalMapping::CreateNewMapPoints: the restatement and the emulated kernels against the fixtures under
tests/golden/new_points that the reference's own function produced, and that function - cut out of the reference's sources with
Triangulate, UnprojectStereo, unprojectEig and project, compiled unmodified (tests/new_points_golden.py), its
SearchForTriangulation the reference's own ORBmatcher.cc - against the fixtures and against the restatement on fresh seeds.
This pins the control flow, the overload resolution of cos / atan2 and the order of the tests; not the SVD or Eigen's
evaluation order (tests/new_points_ref_types.h)."""
import numpy as np
import pytest

import new_points_golden as ng
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

needs_reference = pytest.mark.skipif(not ng.have_reference(), reason="the reference sources or oracle/_ref are not on this machine")
AT_LEAST = dict(main=300, inertial=100, monocular=100)


@pytest.mark.parametrize("name", sorted(ng.CASES))
def test_restatement_and_emulated_kernels_match_golden(emu_lib, name):
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    assert ng.assert_matches_golden(name, ng.restatement_backend(mt)) >= AT_LEAST[name]
    assert ng.assert_matches_golden(name, ng.device_backend(mt)) >= AT_LEAST[name]
    mt.close()


def test_fixture_conditions(emu_lib):
    """what the fixtures have to contain: a neighbour left out by the baseline test (main) and by the monocular median-depth test,
    accepted points of all three kinds, the far-point threshold met exactly, and the two SVD maxima of the accuracy check"""
    import new_points_checks as nc
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    case, fx = ng.fixture_case("main")
    recs, per, _ = mt.CreateNewMapPointsRestatement(nc.oracle_search, case["kf1"], case["neighbours"], dict(case["prm"], report_rejected=1), case["skip"])
    assert ng.encode(recs[np.isin(recs["status"], nc.ACCEPTED)]) == fx["results"]   # ... so these are conditions on the recorded results
    counts = {s: int((recs["status"] == s).sum()) for s in range(14)}
    assert all(counts[s] >= 3 for s in nc.STATUSES_IN_FIXTURE), counts
    assert per[1] == -1 and (per[[0, 3, 4]] > 0).all()
    th = np.float32(case["prm"]["th_far_points"])
    far = recs[recs["status"] == 12]
    Ow1 = np.asarray(case["kf1"]["Ow"], np.float32)
    assert any(nc.f32_norm(r["x3D"] - Ow1) == th for r in far)
    svd = fx["svd"]
    assert svd["triangulated"] >= 200 and svd["max_rel_error_np_triangulate"] <= 4 * svd["max_rel_error_numpy_float32_svd"]
    mono, _ = ng.fixture_case("monocular")
    assert list(mono["skip"]) == [0, 1, 0, 0, 0]
    mt.close()
    for name in ng.CASES:
        import os
        assert os.path.getsize(os.path.join(ng.GOLDEN, name + ".json")) <= 16 * 1024


@needs_reference
@pytest.mark.parametrize("name", sorted(ng.CASES))
def test_reference_code_reproduces_golden(name):
    """The committed fixtures are what src/LocalMapping.cc:388-712, compiled unmodified, leaves in mlpRecentAddedMapPoints; and the
    recorded geometry is what the Sophus stand-in makes of the generated poses."""
    lib = ng.build_reference_glue()
    ng.assert_matches_golden(name, lambda case: ng.reference_results(lib, name, case))
    fx = ng.load(name)
    poses, pairs = ng.reference_geometry(lib, ng.make_case(name, None))
    assert ng.hexf(poses) == fx["poses"] and ng.hexf(pairs) == fx["pairs"]


@needs_reference
def test_restatement_equals_reference_code_on_fresh_seeds(emu_lib):
    lib = ng.build_reference_glue()
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    total = 0
    for seed, kw in ((41, {}), (42, dict(inertial=1)), (43, dict(th_far_points=40.0))):
        ng.CASES["fresh"] = dict(n=400, n_neigh=6, seed=seed, **{k: v for k, v in kw.items() if k != "th_far_points"})
        try:
            geometry = ng.reference_geometry(lib, ng.make_case("fresh", None))
            case = ng.make_case("fresh", geometry, kw.get("th_far_points"))
            rec = ng.reference_results(lib, "fresh", case)
            assert ng.encode(ng.restatement_backend(mt)(case)) == ng.encode(rec), "seed %d" % seed
            total += len(rec)
        finally:
            del ng.CASES["fresh"]
    mt.close()
    assert total > 400
