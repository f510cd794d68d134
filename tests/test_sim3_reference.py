"""Sim3Solver's control flow against the reference's own code.  The fixtures under tests/golden/sim3 are what include/Sim3Solver.h
and src/Sim3Solver.cc - copied without their #include lines and compiled unmodified against tests/sim3_ref_types.h, with the
reference's DUtils::Random over rand() after srand(seed) (tests/sim3_golden.py) - did on generated cases: the triples drawn,
and per call of iterate(20, ...) bNoMore, bConverge, nInliers, mnIterations, mnBestInliers, the matrices and vbInliers.  Checked
here: rgbl_sim3_ransac_host on the recorded triples reproduces every call (no reference needed); the reference's code reproduces
the fixtures, and agrees with the host build on fresh seeds (skipped where the reference is absent).
This pins the sampling order, SetRansacParameters' iteration count, the `>=` and `>` rules, the mapping through mvnIndices1, the
N < mRansacMinInliers exit and both overloads across repeated calls; NOT the eigen decomposition, atan2, SO3f::exp or Eigen's
evaluation order (tests/sim3_ref_types.h)."""
import os

import pytest

import sim3_golden as sg

needs_reference = pytest.mark.skipif(not sg.have_reference(), reason="the reference sources are not on this machine")


@pytest.mark.parametrize("name", sorted(sg.CASES))
def test_host_build_reproduces_golden_calls(emu_lib, name):
    fx = sg.load(name)
    assert fx["params"] == sg.CASES[name]
    sg.check_against_host_build(fx, emu_lib)
    assert os.path.getsize(os.path.join(sg.GOLDEN, name + ".json")) <= 16 * 1024


def test_fixture_conditions():
    """what the fixtures have to contain: a convergence in a later call of 20 before that call's last iteration (state carried
    over calls, and the point where the drop-in has drawn further than the reference), a run through to mRansacMaxIts in a call
    cut short by it, mnBestInliers rising between calls, mRansacMinInliers == N, N < mRansacMinInliers, a convergence at once"""
    fx = {name: sg.load(name) for name in sg.CASES}
    c = fx["converges"]["calls"]
    assert len(c) >= 3 and c[-1]["converge"] and 0 < c[-1]["ran"] < sg.STEP and all(k["ran"] == sg.STEP and not k["converge"] for k in c[:-1])
    assert c[-1]["inliers"] > fx["converges"]["params"]["min_inliers"] and len({k["best"] for k in c}) >= 3
    assert c[-1]["iterations"] == sg.STEP * (len(c) - 1) + c[-1]["ran"]
    r = fx["runs_through"]
    assert r["max_its"] == 169 and len(r["calls"]) == 9 and r["calls"][-1]["ran"] == 9 and r["calls"][-1]["no_more"] and not r["calls"][-1]["converge"]
    assert all(k["best"] <= r["params"]["min_inliers"] for k in r["calls"])
    m = fx["min_equals_n"]
    assert m["max_its"] == 1 and [k["ran"] for k in m["calls"]] == [1] and m["calls"][0]["no_more"]
    t = fx["too_few"]
    assert t["N"] < t["params"]["min_inliers"] and [k["ran"] for k in t["calls"]] == [0]
    a = fx["at_once"]["calls"]
    assert len(a) == 1 and a[0]["converge"] and a[0]["ran"] < sg.STEP
    # the triples are distinct indices into 0 .. N - 1
    for f in fx.values():
        for k in f["calls"]:
            for i in range(0, len(k["triples"]), 3):
                tr = k["triples"][i:i + 3]
                assert len(set(tr)) == 3 and all(0 <= v < f["N"] for v in tr)


@needs_reference
@pytest.mark.parametrize("name", sorted(sg.CASES))
def test_reference_code_reproduces_golden(name):
    """the committed fixtures are what src/Sim3Solver.cc, compiled unmodified, does after srand(seed)"""
    assert sg.reference_run(sg.build_reference(), sg.CASES[name]) == sg.load(name)


@needs_reference
def test_host_build_equals_reference_code_on_fresh_seeds(emu_lib):
    exe = sg.build_reference()
    seen = []
    for seed, fix, mi, share in ((41, 0, 12, 0.7), (42, 1, 20, 0.8), (43, 0, 8, 0.5), (44, 1, 25, 0.95)):
        fx = sg.reference_run(exe, dict(seed=seed, n=80, fix_scale=fix, min_inliers=mi, outlier_share=share))
        seen.append(sg.check_against_host_build(fx, emu_lib))
    assert any(conv for _, conv in seen) and sum(calls for calls, _ in seen) >= 6, seen
