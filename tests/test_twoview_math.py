"""csrc/twoview_math.h (its host build, rgbl_two_view_reconstruct_host) against the float64 numpy model of tests/twoview_model.py - a
second reading of src/TwoViewReconstruction.cc, not the reference - within the tolerance recorded under tests/golden/two_view
(16 x the model's own float32 / float64 difference, measured on the model alone), and the stand-alone sanitizer program
tests/twoview_host_check.cpp."""
import json
import os
import subprocess

import numpy as np
import pytest

import twoview_model as tmod
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import twoview_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
# KITTI camera, 20 % outliers, 0.3 px of noise, 200 sets (the planar scenes: no outliers)
CASES = {"general_100": ("general", 100, 19), "general_300": ("general", 300, 12), "forward_100": ("forward", 100, 13),
         "planar_100": ("planar", 100, 14), "planar_300": ("planar", 300, 15)}
GPU_CASE = "general_100"
CAPS = {"general": {"F": 0.70, "H": 0.95}, "forward": {"F": 0.70, "H": 0.95}, "planar": {"H": 0.95}}


def case_problem(name):
    scene, N, seed = CASES[name]
    return tc.problem(tc.make_two_view_case(N, 200, seed=seed, scene=scene, pixel_noise=0.3, outlier_share=0.0 if scene == "planar" else 0.2))


def load_recorded():
    with open(os.path.join(tmod.GOLDEN, "tolerance.json")) as fh:
        return json.load(fh)


_models = {}


def model_of(name):
    """the model's float64 run and its noise against the float32 run, once per case"""
    if name not in _models:
        _models[name] = tmod.noise(case_problem(name))
    return _models[name]


def compare(got, name, rec, what):
    fwd, own = model_of(name)
    scene = CASES[name][0]
    worst = {}
    for md, key in ((0, "H"), (1, "F")):
        keep = fwd["ratio"][:, md] >= rec["ratio"]
        if key in CAPS[scene]:
            assert keep.mean() >= CAPS[scene][key], (what, key, "only %.0f %% of the hypotheses are compared" % (100 * keep.mean()))
        d = np.array([np.abs(tmod.unit(got["models"][k, md]) - tmod.unit(fwd[key][k])).max() for k in np.nonzero(keep)[0]])
        worst[key] = float(d.max()) if len(d) else 0.0
        print("%s %s: %d of %d compared, distance %.3g, tolerance %.3g" % (what, key, keep.sum(), len(keep), worst[key], rec[key + "_tolerance"]))
        assert worst[key] <= rec[key + "_tolerance"], (what, key, worst[key], rec[key + "_tolerance"], int(np.nonzero(keep)[0][np.argmax(d)]))
    # the winners, the choice and the outcome, unless the model's own two runs disagree or its two best scores are within the margin
    decided = own["same_decision"]
    for md, key, best in ((0, "H", "best_h"), (1, "F", "best_f")):
        sc = np.sort(np.nan_to_num(fwd["scores"][:, md]))[::-1]
        decided = decided and (len(sc) < 2 or sc[0] - sc[1] > rec[key + "_score_margin"])
    if decided:
        assert (got["best_h"], got["best_f"], got["model"], got["found"]) == (fwd["best_h"], fwd["best_f"], fwd["model"], fwd["found"]), (what, fwd["SH"], fwd["SF"])
        # n_good as a multiset - which of R1 / R2 and of +-t comes first follows the singular vectors' signs, which are not pinned -
        # equal but for the matches whose squared reprojection error lies within 5 % of th2 in the model
        gap = np.abs(np.sort(got["n_good"]) - np.sort(fwd["n_good"])).sum()
        assert gap <= fwd["near"].sum(), (what, got["n_good"], fwd["n_good"], fwd["near"])
        if fwd["found"]:
            dT = max(np.abs(got["R21"] - fwd["R"]).max(), np.abs(got["t21"] - fwd["t"]).max())
            print("%s T21: distance %.3g, tolerance %.3g" % (what, dT, rec["T21_tolerance"]))
            assert dT <= rec["T21_tolerance"], (what, dT)
    return worst, decided


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_build_against_the_model(emu_lib, name):
    rec = load_recorded()
    got = F.two_view_reconstruct_host(case_problem(name), emu_lib)
    worst, decided = compare(got, name, rec, "host build, case %s" % name)
    assert decided or name.startswith("planar"), "a general scene whose outcome the model itself does not decide checks nothing"


def test_the_recorded_tolerance_is_the_models_noise():
    """tolerance.json holds what the model measures on itself now: the same cases, 16 x the largest difference"""
    rec = load_recorded()
    assert rec["factor"] == 16.0 and rec["ratio"] == tmod.RATIO and sorted(rec["cases"]) == sorted(CASES)
    for key in ("H", "F"):
        now = max(model_of(n)[1][key]["noise"] for n in CASES)
        assert rec[key + "_tolerance"] == 16.0 * rec[key + "_noise"]
        assert 0.25 * rec[key + "_noise"] <= now <= 4.0 * rec[key + "_noise"], (key, now, rec[key + "_noise"])   # LAPACK builds differ in the last bits


def test_recovers_the_planted_motion(emu_lib):
    """an end in itself: the motion is the plant's, the triangulated matches are no planted outliers"""
    case = tc.make_two_view_case(300, 200, seed=21, pixel_noise=0.05)
    got = F.two_view_reconstruct_host(tc.problem(case), emu_lib)
    assert got["found"] == 1 and got["model"] == 1
    t = case["t_true"] / np.linalg.norm(case["t_true"])
    assert np.abs(got["R21"] - case["R_true"]).max() < 5e-3 and np.abs(got["t21"] - t).max() < 2e-2
    # a planted outlier is displaced by 30 - 80 px; one displaced ALONG its epipolar line stays an inlier of any F (about 2 %)
    wrong = int((got["triangulated"][case["idx1"]].astype(bool) & case["planted_outlier"].astype(bool)).sum())
    assert wrong <= 0.1 * case["planted_outlier"].sum(), wrong
    X = got["p3d"][case["idx1"]][got["triangulated"][case["idx1"]] == 1]
    assert len(X) > 150 and (X[:, 2] > 0).all()


def test_stand_alone_host_program_under_sanitizers():
    """tests/twoview_host_check.cpp: the header's acos against libm's, the null vectors against a residual bound, and every
    function on general, planar, coincident, collinear and inf-normalised data, compiled with -fsanitize=address,undefined and
    run here."""
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, "twoview_host_check_%d" % os.getpid()), os.path.join(ROOT, "tests", "twoview_host_check.cpp")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I" + os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc"), src, "-o", exe])
        res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    print(res.stdout)
    assert res.returncode == 0 and "TWOVIEW_HOST_CHECK_OK" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
