"""csrc/mlpnp_math.h on the CPU: the host build (rgbl_mlpnp_ransac_host) against the float64 model of tests/mlpnp_model.py, the
model's analytic Jacobian against central differences, and the stand-alone sanitizer program tests/mlpnp_host_check.cpp.

Tolerance (tests/golden/mlpnp/README.md).  The model is run twice on every case below: with the samples as drawn, and with every
sum over the correspondences of a set taken in the opposite order (the six-sets reversed; the sign tests keep reading the first
six).  That is pure reordering.  A hypothesis is COMPARED when both runs take the same Gauss-Newton path
(updates, break / stop / failed solve) and both poses are finite.  `reordering_noise` is the largest pose difference over the
compared hypotheses - rotation entries absolute, translation relative to the scene's extent -, `tolerance` is FACTOR x that.
`margin_noise` is the largest |e - e'| / (e + threshold) of the squared reprojection errors of the two runs, `margin_bound`
FACTOR x that; a (hypothesis, correspondence) pair is DECIDED when its model error is further from the threshold than
margin_bound x (e + threshold), and inlier flags must be equal on every decided pair.  All of it comes from the model alone;
tests/golden/mlpnp/tolerance.json records it and is what every comparison uses (here and in tests/test_mlpnp_gpu.py);
test_recorded_tolerance_is_the_measured_one re-measures within a factor of 4."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import mlpnp_model as mm
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import mlpnp_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mlpnp")
FACTOR = 16   # the factor of sim3 and sim3_opt: another eigen solver and another summation tree

# (N, seed, outlier share): 300 hypotheses each, outliers displaced by 30 - 80 px, inlier noise 0.3 sigma of the level,
# min_inliers = N / 2.  The seeds are chosen so that the model ALONE meets the caps and the call succeeds at a hypothesis that is
# not among the first three (the scan has hypotheses to pass before it stops).
CASES = [(20, 1, 0.15), (20, 2, 0.3), (100, 1, 0.3), (100, 12, 0.15), (300, 1, 0.3), (300, 3, 0.15)]
GPU_CASE = 2   # N = 100


def make(index):
    N, seed, share = CASES[index]
    return mc.problem(mc.make_mlpnp_case(N, 300, seed=seed, outlier_share=share, min_inliers=N // 2))


@functools.lru_cache(maxsize=None)
def model_runs(index):
    """(problem, the model as drawn, the model reversed); the forward run also carries `compared` and `extent`"""
    pr = make(index)
    fwd, rev = mm.iterate(pr), mm.iterate(pr, reverse=True)
    fwd["extent"] = float(np.abs(np.asarray(pr["world_pos"])).max())
    fwd["compared"] = same_path(fwd, rev)
    return pr, fwd, rev


def load_recorded():
    return json.load(open(os.path.join(GOLDEN, "tolerance.json")))


def same_path(a, b):
    return (a["gn_path"] == b["gn_path"]) & np.isfinite(a["Tcw_all"]).all((1, 2)) & np.isfinite(b["Tcw_all"]).all((1, 2))


def pose_difference(A, B, extent):
    with np.errstate(invalid="ignore"):
        return np.maximum(np.abs(A[..., :3] - B[..., :3]).max((-2, -1)), np.abs(A[..., 3] - B[..., 3]).max(-1) / extent)


def error_difference(e, e2, thr):
    """|e - e'| / (e + threshold); 0 where both are not finite (both are outliers then)"""
    e, e2 = e.astype(np.float64), e2.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(e - e2) / (e + thr)
    return np.where(np.isfinite(e) | np.isfinite(e2), np.nan_to_num(d, nan=np.inf), 0.0)


def decided(e, thr, margin_bound):
    e = e.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return ~np.isfinite(e) | (np.abs(e - thr) > margin_bound * (e + thr))


def thresholds(pr):
    return mm.correspondences(pr)["max_err"].astype(np.float64)


def measure():
    """(reordering_noise, margin_noise) over all cases: the model as drawn against the model reversed"""
    d_t = d_e = 0.0
    for i in range(len(CASES)):
        pr, fwd, rev = model_runs(i)
        cmp, thr = fwd["compared"], thresholds(pr)
        d_t = max(d_t, float(pose_difference(fwd["Tcw_all"], rev["Tcw_all"], fwd["extent"])[cmp].max()))
        d_e = max(d_e, float(error_difference(fwd["err2"], rev["err2"], thr)[cmp].max()))
    return d_t, d_e


def all_flags(mt, pr, host):
    """the flags of every hypothesis with at least six inliers, which one call returns for its record only: one problem per
    hypothesis (a single sample, min_inliers = 6: it becomes the record, and its mask the new state) through the batch form.
    Returns (flags, valid)."""
    S = np.asarray(pr["samples"]).reshape(-1, 6)
    N = int((np.asarray(pr["mp_index"]) >= 0).sum())
    res = mt.MLPnPRansacBatch([dict(pr, samples=S[h:h + 1], n_hyp=1, best_inliers=0, best_mask=None, min_inliers=6) for h in range(len(S))],
                              host=host, diag=False)
    valid = np.array([r["best_inliers"] >= 6 for r in res])
    return np.stack([r["best_mask"][:N] * v for r, v in zip(res, valid)]).astype(bool), valid


def compare(got, fwd, recorded, what, flags=None):
    """a result dict of the library (with diagnostics) against the model's forward run; returns the largest pose difference"""
    cmp = fwd["compared"] & (got["gn_path"] == fwd["gn_path"]) & np.isfinite(got["Tcw_all"]).all((1, 2))
    d = pose_difference(got["Tcw_all"], fwd["Tcw_all"], fwd["extent"])
    worst = float(d[cmp].max())
    print("%s: pose difference %.3g (tolerance %.3g), %d of %d hypotheses compared" % (what, worst, recorded["tolerance"], int(cmp.sum()), len(cmp)))
    assert cmp.mean() >= 0.90, (what, cmp.mean())
    qualifying = fwd["counts"] >= fwd["min_inliers"]
    assert cmp[qualifying].all(), (what, "a hypothesis with count >= min_inliers is not compared")
    assert worst <= recorded["tolerance"], (what, worst)
    dec = decided(fwd["err2"], fwd["thresholds"], recorded["margin_bound"]) & cmp[:, None]
    lo, hi = (fwd["flags"] & dec).sum(1), (fwd["flags"] | ~dec).sum(1)
    c = got["counts"]
    assert ((c[cmp] >= lo[cmp]) & (c[cmp] <= hi[cmp])).all(), (what, "counts outside what the decided pairs allow")
    for k in ("found", "no_more", "iterations_run", "refines"):
        assert got[k] == fwd[k], (what, k, got[k], fwd[k])
    # the returned solution: the hypothesis at which the call stops, in float
    assert fwd["found"] == 1 and fwd["no_more"] == 0 and fwd["selected"] == fwd["iterations_run"] - 1, what
    h = fwd["selected"]
    assert cmp[h], (what, "the returned hypothesis is not a compared one")
    assert np.array_equal(got["Tcw"][:3], got["Tcw_all"][h].astype(np.float32)), (what, "Tcw is not the returned hypothesis in float")
    inl = got["inlier"][fwd["feat"]].astype(bool)
    assert np.array_equal(inl[dec[h]], fwd["flags"][h][dec[h]]), (what, "the flags of the returned hypothesis")
    assert got["n_inliers"] == c[h] == int(inl.sum()), (what, got["n_inliers"])
    if flags is not None:   # every decided pair of every compared hypothesis with six inliers or more
        fl, valid = flags
        assert np.array_equal(valid, c >= 6), what
        assert np.array_equal(fl.sum(1)[valid], c[valid]), (what, "the counts are not the sums of the flags")
        sel = dec & valid[:, None]
        assert np.array_equal(fl[sel], fwd["flags"][sel]), (what, int((fl[sel] != fwd["flags"][sel]).sum()))
    return worst


def prepared(index):
    pr, fwd, rev = model_runs(index)
    fwd.setdefault("thresholds", thresholds(pr))
    fwd.setdefault("min_inliers", int(pr["min_inliers"]))
    fwd.setdefault("feat", mm.correspondences(pr)["feat"])
    return pr, fwd, rev


def test_jacobian_against_central_differences():
    """the model's analytic Jacobian (the header derives the same expressions) against central differences of the residuals"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        f = np.c_[rng.uniform(-0.8, 0.8, (7, 2)), np.ones(7)]
        X = rng.uniform(-5, 5, (7, 3)) + np.array([0, 0, 12.0])
        x = np.r_[rng.normal(size=3) * rng.uniform(0.01, 1.5), rng.uniform(-2, 2, 3)]
        J = mm.jacobian(x, f, X)
        h = 1e-6
        for k in range(6):
            e = np.zeros(6)
            e[k] = h
            num = (mm.residuals(x + e, f, X) - mm.residuals(x - e, f, X)) / (2 * h)
            assert np.abs(J[:, :, k] - num).max() < 1e-8, (k, np.abs(J[:, :, k] - num).max())
    assert np.isnan(mm.jacobian(np.r_[0.0, 0.0, 0.0, 0.1, 0.2, 0.3], f, X)).any()   # the singularity at w = 0 is kept


def test_recorded_tolerance_is_the_measured_one():
    recorded = load_recorded()
    d_t, d_e = measure()
    print("model as drawn against model reversed: pose %.3g (recorded %.3g), squared errors %.3g (recorded %.3g)"
          % (d_t, recorded["reordering_noise"], d_e, recorded["margin_noise"]))
    assert recorded["factor"] == FACTOR and recorded["tolerance"] == FACTOR * recorded["reordering_noise"]
    assert recorded["margin_bound"] == FACTOR * recorded["margin_noise"]
    assert [list(c) for c in CASES] == recorded["cases"]
    # numpy's LAPACK / BLAS kernels depend on the CPU: the recorded numbers have to be this machine's within a factor of 4
    assert recorded["reordering_noise"] / 4 <= d_t <= recorded["reordering_noise"] * 4
    assert recorded["margin_noise"] / 4 <= d_e <= recorded["margin_noise"] * 4


def test_model_alone_meets_the_caps():
    recorded = load_recorded()
    for i in range(len(CASES)):
        pr, fwd, rev = prepared(i)
        cmp = fwd["compared"]
        dec = decided(fwd["err2"], fwd["thresholds"], recorded["margin_bound"])
        left_out = 1.0 - dec.mean()
        qualifying = fwd["counts"] >= fwd["min_inliers"]
        print("case %s: %.1f %% of the hypotheses compared, %d qualifying all compared, %.3f %% of the pairs undecided, success at hypothesis %d"
              % (CASES[i], 100 * cmp.mean(), int(qualifying.sum()), 100 * left_out, fwd["iterations_run"] - 1))
        assert cmp.mean() >= 0.90, (CASES[i], cmp.mean())
        assert cmp[qualifying].all(), CASES[i]
        assert left_out <= 0.02, (CASES[i], left_out)
        # the call succeeds at a hypothesis that is not among the first three, in both runs alike
        assert fwd["found"] == rev["found"] == 1 and fwd["no_more"] == 0 and fwd["iterations_run"] == rev["iterations_run"] > 3, CASES[i]
        assert np.array_equal(fwd["flags"][dec & cmp[:, None]], rev["flags"][dec & cmp[:, None]]), CASES[i]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_host_build_against_the_model(emu_lib, index):
    pr, fwd, _ = prepared(index)
    got = F.mlpnp_ransac_host(pr, emu_lib)
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    compare(got, fwd, load_recorded(), "host build, case %s" % (CASES[index],), all_flags(mt, pr, host=True))
    mt.close()
    assert got["n_inliers"] == int(got["inlier"].sum())


def test_recovers_the_planted_pose(emu_lib):
    """an end in itself: the six-point hypothesis the call stops at is close to the plant and separates the planted outliers"""
    case = mc.make_mlpnp_case(300, 35, seed=5, min_inliers=150)
    got = F.mlpnp_ransac_host(mc.problem(case), emu_lib)
    assert got["found"] == 1 and got["no_more"] == 0
    assert np.abs(got["Tcw"][:3, :3] - case["R_true"]).max() < 0.01 and np.abs(got["Tcw"][:3, 3] - case["t_true"]).max() < 0.2
    assert not (got["inlier"][case["feat"]].astype(bool) & case["planted_outlier"].astype(bool)).any()


def test_stand_alone_host_program_under_sanitizers():
    """tests/mlpnp_host_check.cpp: the header's host build on seeded, planar and degenerate sets (coincident and collinear
    points, non-finite coordinates, an identity pose), the rank rule, the cube root, acos and the scan's corners, compiled with
    -fsanitize=address,undefined and run here."""
    os.makedirs(BUILD, exist_ok=True)
    exe, src = os.path.join(BUILD, "mlpnp_host_check_%d" % os.getpid()), os.path.join(ROOT, "tests", "mlpnp_host_check.cpp")
    try:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I" + os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc"), src, "-o", exe])
        res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    finally:
        if os.path.exists(exe):
            os.remove(exe)
    print(res.stdout)
    assert res.returncode == 0 and "MLPNP_HOST_CHECK_OK" in res.stdout, res.stdout + res.stderr
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
