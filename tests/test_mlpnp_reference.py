"""MLPnPsolver's control flow against the reference's own code.  The fixtures under tests/golden/mlpnp are what the reference's
constructor, iterate, SetRansacParameters, CheckInliers, Refine and Pinhole::project / unproject - cut out by signature and compiled
unmodified against tests/mlpnp_ref_types.h, with the reference's DUtils::Random over rand() after srand(seed)
(tests/mlpnp_golden.py) - did on generated cases: the sets drawn, and per call of iterate(5, ...) the return value, bNoMore,
nInliers, mnIterations, mnBestInliers, Tout, mBestTcw and vbInliers.  Checked here: rgbl_mlpnp_ransac_host on the recorded sets
reproduces every call bit for bit (no reference needed); the reference's code reproduces the fixtures, and agrees with the host
build on fresh seeds (skipped where the reference is absent).
This pins the constructor's bookkeeping, SetRansacParameters, the sampling order, the `||` of the loop condition, the `>=` and `>`
rules, what Refine returns as compiled and the mapping through mvKeyPointIndices; NOT computePose, which cannot be compiled
without Eigen and forwards to csrc/mlpnp_math.h in the stand-in (tests/mlpnp_ref_types.h): that is the model's."""
import os

import numpy as np
import pytest

import mlpnp_golden as mg

needs_reference = pytest.mark.skipif(not mg.have_reference(), reason="the reference sources are not on this machine")


@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_host_build_reproduces_golden_calls(emu_lib, name):
    fx = mg.load(name)
    assert fx["params"] == mg.CASES[name]
    mg.check_against_host_build(fx, emu_lib)
    assert os.path.getsize(os.path.join(mg.GOLDEN, name + ".json")) <= 16 * 1024


def test_fixture_conditions(emu_lib):
    """what the fixtures have to contain.  The counts of the hypotheses are the host build's on the recorded sets (the reference
    keeps only the last one); check_against_host_build has held every recorded figure against them."""
    fx = {name: mg.load(name) for name in mg.CASES}
    counts = {name: mg.check_against_host_build(fx[name], emu_lib) for name in mg.CASES}
    # success at the first qualifying hypothesis, after hypotheses that do not qualify
    f, c = fx["first_qualifying"], counts["first_qualifying"][0]
    assert len(f["calls"]) == 1 and f["calls"][0]["ret"] and not f["calls"][0]["no_more"] and f["calls"][0]["ran"] > 3
    assert (c[:-1] < f["min_inliers"]).all() and c[-1] == f["calls"][0]["inliers"] > f["min_inliers"]
    # a failed Refine (count == mRansacMinInliers: `>` is strict) before a success; Refine ran twice
    f, c = fx["failed_refine"], counts["failed_refine"][0]
    q = c[c >= f["min_inliers"]]
    assert list(q[:-1]) == [f["min_inliers"]] * (len(q) - 1) and len(q) >= 2 and q[-1] > f["min_inliers"] and f["refine_poses"] == len(q)
    assert f["calls"][0]["ret"] and not f["calls"][0]["no_more"] and f["calls"][0]["inliers"] == q[-1]
    # a run-through that returns mBestTcw: the best is exactly mRansacMinInliers
    f = fx["best_after_run_through"]
    last = f["calls"][-1]
    assert last["ret"] and last["no_more"] and last["inliers"] == last["best"] == f["min_inliers"] and last["T"] == last["best_Tcw"]
    assert last["iterations"] == f["max_its"] and f["refine_poses"] >= 1
    # a run-through that returns false: the first call of iterate(5) runs all mRansacMaxIts iterations (the `||`)
    f = fx["runs_through"]
    assert [(k["ran"], k["ret"], k["no_more"], k["best"]) for k in f["calls"]] == [(f["max_its"], 0, 1, 0)] and f["max_its"] > mg.STEP
    assert f["calls"][0]["T"] == mg.IDENTITY and f["refine_poses"] == 0
    # N < mRansacMinInliers
    f = fx["too_few"]
    assert f["N"] < f["min_inliers"] and [(k["ran"], k["ret"], k["no_more"]) for k in f["calls"]] == [(0, 0, 1)] and f["six_point_poses"] == 0
    # mRansacMinInliers == N: mRansacMaxIts is 1, yet iterate(5) runs 5 iterations
    f = fx["min_equals_n"]
    assert f["min_inliers"] == f["N"] and f["max_its"] == 1 and [k["ran"] for k in f["calls"]] == [mg.STEP] and f["calls"][0]["no_more"]
    # a second call after a success: the loop goes on drawing; what it returns is the hypothesis it stops at, not the first call's
    f = fx["second_call"]
    a, b = f["calls"]
    assert a["ret"] and b["ret"] and not a["no_more"] and b["iterations"] == a["iterations"] + b["ran"] and b["best"] >= a["best"]
    assert a["sets"][-6:] != b["sets"][-6:]
    # Refine's computePose is answered with NaN by the stand-in: nothing recorded anywhere is a NaN, so its result is never read
    for name, f in fx.items():
        assert all("7fc00000" not in k["T"] and "7fc00000" not in k["best_Tcw"] for k in f["calls"]), name
    assert sum(f["refine_poses"] for f in fx.values()) >= 8


@needs_reference
@pytest.mark.parametrize("name", sorted(mg.CASES))
def test_reference_reproduces_fixtures(name):
    exe = mg.build_reference()
    assert mg.reference_run(exe, mg.CASES[name]) == mg.load(name)


@needs_reference
def test_reference_agrees_with_host_build_on_fresh_seeds(emu_lib):
    exe = mg.build_reference()
    rng = np.random.default_rng(77)
    outcomes = set()
    for seed in range(100, 112):
        params = dict(seed=seed, N=int(rng.integers(12, 80)), min_inliers=10, outlier_share=float(rng.choice([0.2, 0.5, 0.7])),
                      pixel_noise=0.3, after_success=int(rng.integers(0, 3)))
        fx = mg.reference_run(exe, params)
        mg.check_against_host_build(fx, emu_lib)
        outcomes.add((fx["calls"][-1]["ret"], fx["calls"][-1]["no_more"]))
    assert len(outcomes) >= 2, outcomes
