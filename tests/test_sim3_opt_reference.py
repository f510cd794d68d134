"""OptimizeSim3's control flow against the reference's own lines.  The fixtures under tests/golden/sim3_opt are what
src/Optimizer.cc:2115-2381 - copied at test time and compiled unmodified against tests/sim3_opt_ref_types.h
(tests/sim3_opt_golden.py) - did on generated cases: the return value, the edge pairs of the set-up loop with obs2 and its
information, every optimize() call, g2oS12, mAcumHessian and the cleared matches.  Checked here: rgbl_optimize_sim3_host
reproduces every fixture bit for bit (no reference needed); the reference's lines reproduce the fixtures, and agree with the host
build on fresh seeds (skipped where the reference is absent).
This pins the set-up loop, obs2 and its level, which pairs are dropped, nMoreIterations, the early return and the final loop;
NOT g2o's arithmetic (tests/sim3_opt_ref_types.h)."""
import os

import numpy as np
import pytest

import sim3_opt_golden as og

needs_reference = pytest.mark.skipif(not og.have_reference(), reason="the reference sources are not on this machine")


@pytest.mark.parametrize("name", sorted(og.CASES))
def test_host_build_reproduces_golden_run(emu_lib, name):
    fx = og.load(name)
    assert fx["params"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in og.CASES[name].items()}
    og.check_against_host_build(fx, emu_lib)
    assert os.path.getsize(os.path.join(og.GOLDEN, name + ".json")) <= 16 * 1024


def test_fixture_conditions(emu_lib):
    """what the fixtures have to contain: matches not observed in key frame 2 with and without bAllPoints, their inverse edge on
    level 0 with a normalised observation; null and bad points; the return at :2349 with 9 survivors and its other side with 10;
    10 more iterations after a drop, of which more than 5 run; 5 when none was dropped; a point behind and one on the camera
    plane; no edge at all"""
    fx = {name: og.load(name) for name in og.CASES}
    a, b = fx["all_points"], fx["not_all_points"]
    assert a["pairs"] == 162 and b["pairs"] == 135 and a["optimize"][1][0] == 10
    info2 = np.frombuffer(bytes.fromhex(a["info2"]), ">u4").astype("<u4").view(np.float32)
    obs2 = np.frombuffer(bytes.fromhex(a["obs2"]), ">u4").astype("<u4").view(np.float32).reshape(-1, 2)
    normalised = np.abs(obs2).max(1) < 2.0
    assert int(normalised.sum()) == 27 and (info2[normalised] == 1.0).all() and len(set(info2[~normalised])) > 4
    assert fx["nine_survive"]["result"] == 0 and len(fx["nine_survive"]["optimize"]) == 1 and not fx["nine_survive"]["hessian_zeroed"]
    assert fx["ten_survive"]["result"] == 10 and fx["ten_survive"]["optimize"][1][:2] == [10, 10] and fx["ten_survive"]["hessian_zeroed"]
    assert fx["ten_iterations"]["optimize"][1][0] == 10 and fx["ten_iterations"]["optimize"][1][3] > 5
    assert fx["none_dropped"]["optimize"][1] == [5, 30, 0, 5]
    assert fx["depth"]["pairs"] == 57 and fx["no_edge"]["pairs"] == 0 and fx["no_edge"]["optimize"] == [[5, 0, 0, 0]]
    assert fx["fix_scale"]["estimate"][-16:] == np.float64(1.0).tobytes().hex()


@needs_reference
@pytest.mark.parametrize("name", sorted(og.CASES))
def test_reference_lines_reproduce_golden(name):
    """the committed fixtures are what Optimizer.cc:2115-2381, compiled unmodified, does"""
    assert og.reference_run(og.build_reference(), og.CASES[name]) == og.load(name)


@needs_reference
def test_host_build_equals_reference_lines_on_fresh_seeds(emu_lib):
    exe = og.build_reference()
    rounds = []
    for seed, fix, share, everything in ((41, False, 0.1, True), (42, True, 0.0, False), (43, False, 0.3, True), (44, True, 0.2, False)):
        params = dict(n=150, matched=90, seed=seed, fix_scale=fix, out_kf2_share=share, all_points=everything, bad_share=0.05, null_mp1_share=0.05,
                      displace=seed % 3)
        rounds.append(og.check_against_host_build(og.reference_run(exe, params), emu_lib)["rounds"])
    assert 2 in rounds, rounds
