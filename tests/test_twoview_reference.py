"""rgbl_two_view_reconstruct_host (the host build of csrc/twoview_math.h) against the reference's OWN TwoViewReconstruction functions
(tests/twoview_golden.py: cut by signature, compiled unmodified against tests/twoview_ref_types.h): the recorded runs under
tests/golden/two_view are reproduced bit for bit from the committed data alone; where the reference sources are present they are
compiled and must reproduce the fixtures, and agree with the host build on fresh seeds."""
import json

import pytest

import twoview_golden as tg
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import twoview_cases as tc

needs_reference = pytest.mark.skipif(not tg.have_reference(), reason="the reference sources are not on this machine")


@pytest.mark.parametrize("name", sorted(tg.CASES))
def test_host_build_reproduces_the_recorded_run(emu_lib, name):
    fx = tg.load(name)
    assert fx["params"] == json.loads(json.dumps(tg.CASES[name]))
    res = tg.check_against_host_build(fx, emu_lib)
    assert (res[-1]["model"], res[-1]["exit_code"]) == tuple(tg.CASES[name]["last"]), (res[-1]["model"], res[-1]["exit_code"])


def test_fixture_conditions(emu_lib):
    """the seven cases the recorded runs must hold, and the overload of acos at :895"""
    res = {name: tg.check_against_host_build(tg.load(name), emu_lib) for name in tg.CASES}
    fx = {name: tg.load(name) for name in tg.CASES}
    assert fx["f_success"]["calls"][0]["ret"] == 1 and fx["f_success"]["calls"][0]["p3d_size"] == 120
    h = fx["h_success"]["calls"][1]
    assert h["ret"] == 1 and h["p3d_size"] == 0 and res["h_success"][1]["p3d_assigned"] == 0 and res["h_success"][1]["model"] == 0   # ReconstructH drops bestP3D
    ns = res["f_nsimilar"][0]
    assert ns["aux"] == 2 and ns["n_good"].max() == 100 and fx["f_nsimilar"]["calls"][0]["ret"] == 0            # not too few: nsimilar
    fp = res["f_parallax"][0]
    assert fp["aux"] == 1 and fp["n_good"][fp["best_motion"]] >= 50 and fp["parallax"][fp["best_motion"]] <= 1.0
    hs = res["h_second_best"][0]
    assert hs["model"] == 0 and hs["aux"] >= 0.75 * hs["n_good"].max() and fx["h_second_best"]["calls"][0]["ret"] == 0
    z = fx["no_score"]["calls"][0]
    assert z["ret"] == 0 and z["mask_f_size"] == 0 and z["mask_h_size"] == 100 and z["SH"] == "00000000" and z["SF"] == "00000000"   # :185: the F mask stays EMPTY
    one = res["sh_zero"][0]
    assert one["SH"] == 0 and one["best_h"] == -1 and one["SF"] > 0 and one["found"] == 1
    # a second call on the same object: the stream of rand() goes on (the sets differ from the first call's)
    assert fx["f_200"]["calls"][0]["sets"] != fx["f_200"]["calls"][1]["sets"] and len(fx["f_200"]["calls"][0]["sets"]) == 1600
    # acos(float) under the using-directive binds the float overload, in every run that reaches :895
    assert all(f["acos_double"] == 0 for f in fx.values()) and sum(f["acos_float"] for f in fx.values()) > 0


def test_recorded_sets_are_glibc_rand(emu_lib):
    """the sets the reference drew are RandomInt's formula over glibc's rand() after srand(0): what twoview_cases.GlibcRand and the
    drop-in's generator restate"""
    for name in tg.CASES:
        fx, rand = tg.load(name), tc.GlibcRand(0)
        for call in fx["calls"]:
            assert call["sets"] == tc.draw_sets(100, fx["params"]["iterations"], rand).reshape(-1).tolist(), name


@needs_reference
def test_reference_reproduces_the_fixtures():
    exe = tg.build_reference()
    for name, params in tg.CASES.items():
        got, fx = tg.reference_run(exe, params), tg.load(name)
        assert got["calls"] == fx["calls"] and (got["acos_float"], got["acos_double"]) == (fx["acos_float"], fx["acos_double"]), name


@needs_reference
def test_reference_agrees_with_the_host_build_on_fresh_seeds(emu_lib):
    exe = tg.build_reference()
    taken = set()
    for seed in range(40, 52):
        scene = tc.SCENES[seed % len(tc.SCENES)]
        kw = dict(seed=seed, scene=scene, pixel_noise=(0.0, 0.1, 0.3)[seed % 3])
        if scene in ("planar", "rotation", "mirror"):
            kw["outlier_share"] = 0.0
        params = dict(iterations=(2, 8, 60)[(seed // 3) % 3], sigma=1.0, calls=[kw, dict(kw, seed=seed + 100)], last=None)
        for r in tg.check_against_host_build(tg.reference_run(exe, params), emu_lib):
            taken.add((r["model"], r["exit_code"]))
    assert len(taken) >= 3, taken      # successes and both kinds of ReconstructF's rejections at the least
