"""csrc/sim3_math.h on the CPU: the host build (rgbl_sim3_ransac_host) against the float64 model of tests/sim3_model.py, and
the stand-alone sanitizer program tests/sim3_host_check.cpp.

Tolerance (tests/golden/sim3/README.md).  The model is run in float32 and in float64 on every case below; over the hypotheses
the model calls well conditioned, `float_difference` is the largest difference of any entry of sR / s, of s (relative) and of
t (relative to the scene's extent), and `tolerance` is 16 x that: the factor covers another evaluation order and another eigen
solver in fp32.  `margin_float_difference` is the largest relative difference of the squared errors, `margin_bound` 16 x that.
Both come from the model alone; tests/golden/sim3/tolerance.json records them and is what every comparison uses (here and in
tests/test_sim3_gpu.py); test_recorded_tolerance_is_the_measured_one re-measures within a factor of 4.

Inlier flags must be EQUAL for every (hypothesis, correspondence) pair whose float64 error is further than margin_bound
(relative) from its threshold; at least 90 % of a case's hypotheses are compared and at most 2 % of its pairs are left out -
asserted for the model alone, as is that its `selected` does not depend on the pairs left out."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sim3_model as sm
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import sim3_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3")

# (n, seed, fix_scale): 300 hypotheses each, 30 % outliers displaced by 30 - 80 px, inlier noise 0.3 sigma of the level
# the seeds are chosen so that the model ALONE meets the caps and its selected hypothesis is a compared one that is not among the
# first three (the scan has updates to make before it stops)
CASES = [(20, 2, 0), (20, 14, 1), (100, 8, 0), (100, 7, 1), (300, 2, 0), (300, 9, 1)]
GPU_CASE = 2   # n = 100


def make(index):
    n, seed, fix = CASES[index]
    return sc.problem(sc.make_sim3_case(n, 300, seed=seed, fix_scale=fix, min_inliers=n // 2))


@pytest.fixture(scope="module")
def modelled():
    """every case with the model's two runs: [(problem, float64 run, float32 run)]"""
    out = []
    for i in range(len(CASES)):
        pr = make(i)
        out.append((pr, sm.run(pr, np.float64), sm.run(pr, np.float32)))
    return out


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "tolerance.json")))


def measure(modelled):
    """(float_difference, margin_float_difference) over all cases: model float32 against model float64"""
    d_t = d_e = 0.0
    for pr, m64, m32 in modelled:
        cmp = m64["compared"]
        d = sm.transform_difference(m32["R"], m32["t"], m32["s"], m64["R"], m64["t"], m64["s"], m64["extent"])
        d_t = max(d_t, float(d[cmp].max()))
        for k, thr in (("err1", "e1"), ("err2", "e2")):
            d_e = max(d_e, float(sm.error_difference(m32[k], m64[k], m64[thr])[cmp].max()))
    return d_t, d_e


def all_flags(mt, pr, host):
    """the flags of EVERY hypothesis, which one call returns for the selected one only: one problem per hypothesis (a single
    sample triple, nothing to beat and no early stop: it is selected) through the batch form in one call"""
    S = np.asarray(pr["samples"]).reshape(-1, 3)
    n = len(np.asarray(pr["max_err1"]))
    res = mt.Sim3RansacBatch([dict(pr, samples=S[h:h + 1], n_hyp=1, best_inliers=0, min_inliers=n) for h in range(len(S))], host=host, diag=False)
    assert all(r["selected"] == 0 for r in res)
    return np.stack([r["inlier"] for r in res]).astype(bool)


def compare(got, m64, recorded, what, flags=None):
    """a result dict of the library (with diagnostics) against the float64 run; returns the figures"""
    cmp = m64["compared"]
    T = got["T12_all"].reshape(-1, 4, 4).astype(np.float64)
    sR, t = T[:, :3, :3], T[:, :3, 3]
    with np.errstate(all="ignore"):
        s = np.cbrt(np.linalg.det(np.where(np.isfinite(sR), sR, 0)))
        d = sm.transform_difference(sR / s[:, None, None], t, s, m64["R"], m64["t"], m64["s"], m64["extent"])
    worst = float(d[cmp].max())
    dec = sm.decided(m64, recorded["margin_bound"]) & cmp[:, None]
    lo = (m64["inlier"] & dec).sum(1)
    hi = (m64["inlier"] | ~dec).sum(1)
    print("%s: transformation difference %.3g (tolerance %.3g), %d of %d hypotheses compared" % (what, worst, recorded["tolerance"], int(cmp.sum()), len(cmp)))
    assert worst <= recorded["tolerance"], (what, worst)
    c = got["counts"]
    assert ((c[cmp] >= lo[cmp]) & (c[cmp] <= hi[cmp])).all(), (what, "counts outside what the decided pairs allow")
    for k in ("selected", "converged", "iterations_run"):
        assert got[k] == m64[k], (what, k, got[k], m64[k])
    # the flags of the selected hypothesis (the only ones the interface returns per correspondence)
    h = m64["selected"]
    assert cmp[h], (what, "the selected hypothesis is not a compared one")
    assert np.array_equal(got["inlier"].astype(bool)[dec[h]], m64["inlier"][h][dec[h]]), what
    if flags is not None:   # every decided pair of every compared hypothesis
        assert np.array_equal(flags.sum(1), c), (what, "the counts are not the sums of the flags")
        assert np.array_equal(flags[dec], m64["inlier"][dec]), (what, int((flags[dec] != m64["inlier"][dec]).sum()))
    return worst


def test_recorded_tolerance_is_the_measured_one(modelled, recorded):
    d_t, d_e = measure(modelled)
    print("float32 against float64 model: transformation %.3g (recorded %.3g), squared errors %.3g (recorded %.3g)"
          % (d_t, recorded["float_difference"], d_e, recorded["margin_float_difference"]))
    assert recorded["tolerance"] == sm.FACTOR * recorded["float_difference"]
    assert recorded["margin_bound"] == sm.FACTOR * recorded["margin_float_difference"]
    assert recorded["triangle_bound"] == sm.TRIANGLE_BOUND and recorded["gap_bound"] == sm.GAP_BOUND
    # numpy's LAPACK / BLAS kernels depend on the CPU: the recorded numbers have to be this machine's within a factor of 4
    assert recorded["float_difference"] / 4 <= d_t <= recorded["float_difference"] * 4
    assert recorded["margin_float_difference"] / 4 <= d_e <= recorded["margin_float_difference"] * 4


def test_model_alone_meets_the_caps(modelled, recorded):
    for i, (pr, m64, m32) in enumerate(modelled):
        cmp = m64["compared"]
        share = cmp.mean()
        dec = sm.decided(m64, recorded["margin_bound"])
        left_out = 1.0 - dec.mean()
        print("case %s: %.1f %% of the hypotheses compared, %.3f %% of the pairs left out" % (CASES[i], 100 * share, 100 * left_out))
        assert share >= 0.90, (CASES[i], share)
        assert left_out <= 0.02, (CASES[i], left_out)
        lo, hi = (m64["inlier"] & dec).sum(1), (m64["inlier"] | ~dec).sum(1)
        a = sm.select(lo, 0, pr["min_inliers"])
        b = sm.select(hi, 0, pr["min_inliers"])
        assert a["selected"] == b["selected"] == m64["selected"] >= 0 and a["converged"] == b["converged"] == 1, CASES[i]
        assert cmp[m64["selected"]]
        # the float32 run of the model decides every decided pair as the float64 run does
        assert np.array_equal(m32["inlier"][dec & cmp[:, None]], m64["inlier"][dec & cmp[:, None]]), CASES[i]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_host_build_against_the_model(emu_lib, modelled, recorded, index):
    pr, m64, _ = modelled[index]
    got = F.sim3_ransac_host(pr, emu_lib)
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    compare(got, m64, recorded, "host build, case %s" % (CASES[index],), all_flags(mt, pr, host=True))
    mt.close()
    assert got["n_inliers"] == int(got["inlier"].sum()) == got["counts"][got["selected"]]


def test_recovers_the_planted_similarity(emu_lib):
    """an end in itself: the selected hypothesis is close to the plant and separates the planted outliers"""
    case = sc.make_sim3_case(300, 300, seed=5, fix_scale=False, min_inliers=150)
    got = F.sim3_ransac_host(sc.problem(case), emu_lib)
    assert got["converged"] == 1
    assert np.abs(got["R12"] - case["R_true"]).max() < 0.02 and abs(got["s12"] - case["s_true"]) < 0.02
    assert not (got["inlier"].astype(bool) & case["planted_outlier"].astype(bool)).any()


def test_stand_alone_host_program_under_sanitizers():
    """tests/sim3_host_check.cpp: the header's host build on the degenerate and edge cases (coincident and collinear samples,
    z == 0, non-finite coordinates, the selection scan's corners), compiled with -fsanitize=address,undefined and run here.
    Its atan2 sweep: each of the quotient, the series, the sum with atan(k / 4) and the reflection rounds once, libm's result is
    within 1 ulp of the truth: 4 ulp is the bound."""
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, "sim3_host_check_%d" % os.getpid()), os.path.join(ROOT, "tests", "sim3_host_check.cpp")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I" + os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc"), src, "-o", exe])
        res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    print(res.stdout)
    assert res.returncode == 0 and "SIM3_HOST_CHECK_OK" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    first, every = [float(v) for v in re.search(r"first_quadrant max_ulp ([0-9.]+) all_quadrants max_ulp ([0-9.]+)", res.stdout).groups()]
    assert first <= 4.0 and every <= 4.0
