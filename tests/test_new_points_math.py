"""csrc/newpoint_math.h on the CPU: atanf / atan2f / cos(2 atan2) against the live libm bit for bit (tests/atanf_sweep.cpp), the
one-sided Jacobi SVD of np_triangulate against LAPACK, and every status of the golden main case against a float64 model of
LocalMapping.cc:557-691."""
import ctypes as C
import fcntl
import math
import os
import subprocess

import numpy as np
import pytest

import new_points_checks as nc
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
f32 = np.float32


def sweep_exe():
    exe, src = os.path.join(BUILD, "atanf_sweep"), os.path.join(ROOT, "tests", "atanf_sweep.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("newpoint_math.h", "frustum_math.h", "sincos_glibc.h")]
    os.makedirs(BUILD, exist_ok=True)
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-fno-builtin", src, "-o", exe + ".tmp", "-lm"])
            os.replace(exe + ".tmp", exe)
    return exe


@pytest.mark.parametrize("mode,at_least", [("atan", 239000000), ("atan2", 465000000), ("cos", 70000000)])
def test_atan_restatements_against_libm(mode, at_least):
    res = subprocess.run([sweep_exe(), mode], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " mismatches 0" in res.stdout and int(res.stdout.split()[1]) >= at_least, res.stdout[-3000:]


def rows_of_A(xn1, xn2, T1, T2):
    """GeometricTools.cc:50-53 in fp32"""
    T1, T2 = T1.reshape(3, 4), T2.reshape(3, 4)
    return np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]]).astype(f32)


def unproject(K, xy):
    return np.array([(xy[0] - K[2]) / K[0], (xy[1] - K[3]) / K[1]], f32)


def lapack_x3D(A, dtype):
    v = np.linalg.svd(A.astype(dtype))[2][3]
    return (v[:3] / v[3]).astype(np.float64)


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def model(kf1, kf2, prm, i1, i2):
    """LocalMapping.cc:557-691 in float64 on the fp32 inputs (the SVD: LAPACK's, of the fp32 A).  Returns (status, the least
    relative margin of the comparisons that decided - on 1 - cos for the parallax ones; the depth tests, comparisons with 0, have
    none and are never exempt -,
    and whether the match went to Triangulate)."""
    margins = []

    def less(a, b):
        margins.append(rel(a, b))
        return a < b
    K1, K2 = kf1["K"].astype(np.float64), kf2["K"].astype(np.float64)
    T1, T2 = kf1["Tcw"].reshape(3, 4).astype(np.float64), kf2["Tcw"].reshape(3, 4).astype(np.float64)
    O1, O2 = kf1["Ow"].astype(np.float64), kf2["Ow"].astype(np.float64)
    p1, p2 = kf1["xy"][i1].astype(np.float64), kf2["xy"][i2].astype(np.float64)
    ur1, ur2 = float(kf1["uright"][i1]), float(kf2["uright"][i2])
    s1, s2 = ur1 >= 0, ur2 >= 0
    xn1 = np.array([(p1[0] - K1[2]) / K1[0], (p1[1] - K1[3]) / K1[1], 1.0])
    xn2 = np.array([(p2[0] - K2[2]) / K2[0], (p2[1] - K2[3]) / K2[1], 1.0])
    r1, r2 = T1[:, :3].T @ xn1, T2[:, :3].T @ xn2
    cr = float(r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2)))
    c1 = c2 = cr + 1
    if s1:
        c1 = math.cos(2 * math.atan2(float(kf1["mb"]) / 2, float(kf1["depth"][i1])))
    elif s2:
        c2 = math.cos(2 * math.atan2(float(kf2["mb"]) / 2, float(kf2["depth"][i2])))
    cs = min(c1, c2)
    limit = 0.9996 if prm["inertial"] else 0.9998

    def unproject_stereo(kf, i, T, Ow, Kd):
        z = float(kf["depth"][i])
        if not z > 0:
            return None
        raw = kf["xy_raw"][i].astype(np.float64)
        return T[:, :3].T @ np.array([(raw[0] - Kd[2]) * z / Kd[0], (raw[1] - Kd[3]) * z / Kd[1], z]) + Ow
    if less(1 - cs, 1 - cr) and less(1 - cr, 1.0) and (s1 or s2 or less(1 - limit, 1 - cr)):
        A = rows_of_A(unproject(kf1["K"], kf1["xy"][i1]), unproject(kf2["K"], kf2["xy"][i2]), kf1["Tcw"], kf2["Tcw"])
        v = np.linalg.svd(A.astype(np.float64))[2][3]
        if v[3] == 0:
            return 5, min(margins), True
        x, ok = v[:3] / v[3], 1
    elif s1 and less(1 - c2, 1 - c1):
        x, ok = unproject_stereo(kf1, i1, T1, O1, K1), 2
    elif s2 and less(1 - c1, 1 - c2):
        x, ok = unproject_stereo(kf2, i2, T2, O2, K2), 3
    else:
        return 4, min(margins), False
    if x is None:
        return 6, min(margins), False
    d1, d2 = float(np.linalg.norm(x - O1)), float(np.linalg.norm(x - O2))
    z1 = float(T1[2, :3] @ x + T1[2, 3])
    if z1 <= 0:
        return 7, min(margins), ok == 1
    z2 = float(T2[2, :3] @ x + T2[2, 3])
    if z2 <= 0:
        return 8, min(margins), ok == 1
    mbf = float(kf1["mbf"])
    for st, kf, T, Kd, p, ur, stereo, z, i in ((9, kf1, T1, K1, p1, ur1, s1, z1, i1), (10, kf2, T2, K2, p2, ur2, s2, z2, i2)):
        xc, yc = float(T[0, :3] @ x + T[0, 3]), float(T[1, :3] @ x + T[1, 3])
        u, v = Kd[0] * xc / z + Kd[2], Kd[1] * yc / z + Kd[3]
        sig = float(kf["level_sigma2"][kf["octave"][i]])
        e = (u - p[0]) ** 2 + (v - p[1]) ** 2
        if stereo:
            e += (u - mbf / z - ur) ** 2
        if less((7.8 if stereo else 5.991) * sig, e):
            return st, min(margins), ok == 1
    if d1 == 0 or d2 == 0:
        return 11, min(margins), ok == 1
    if prm["far_points"]:
        th = float(f32(prm["th_far_points"]))
        far1, far2 = not less(d1, th), not less(d2, th)
        if far1 or far2:
            return 12, min(margins), ok == 1
    rd = d2 / d1
    ro = float(kf1["scale_factors"][kf1["octave"][i1]]) / float(kf2["scale_factors"][kf2["octave"][i2]])
    rf = float(f32(prm["ratio_factor"]))
    if less(rd * rf, ro) or less(ro * rf, rd):
        return 13, min(margins), ok == 1
    return ok, min(margins), ok == 1


def svd_maxima(emu_lib, case, recs):
    """(max relative error of x3D of np_triangulate, of numpy's float32 SVD - both against a float64 SVD of the same fp32 A -,
    matches within the 1e-3 margin, matches whose status differs from the float64 model's outside it, triangulated matches)"""
    emu_lib.rgbl_test_np_triangulate.restype = C.c_int
    emu_lib.rgbl_test_np_triangulate.argtypes = [C.c_void_p] * 5
    kf1 = case["kf1"]
    ours, lapack32, close, flipped, n_tri = 0.0, 0.0, 0, [], 0
    T1 = np.ascontiguousarray(kf1["Tcw"], f32)
    for r in recs:
        kf2 = case["neighbours"][r["neighbour"]]["kf"]
        i1, i2 = int(r["idx1"]), int(r["idx2"])
        st, margin, triangulated = model(kf1, kf2, case["prm"], i1, i2)
        if margin < 1e-3:
            close += 1
        elif st != r["status"]:
            flipped.append((i1, i2, int(r["status"]), st, margin))
        if not triangulated or st == 5:
            continue
        xn1, xn2 = unproject(kf1["K"], kf1["xy"][i1]), unproject(kf2["K"], kf2["xy"][i2])
        A = rows_of_A(xn1, xn2, kf1["Tcw"], kf2["Tcw"])
        want = lapack_x3D(A, np.float64)
        got, T2 = np.zeros(3, f32), np.ascontiguousarray(kf2["Tcw"], f32)
        assert emu_lib.rgbl_test_np_triangulate(L.ptr(xn1), L.ptr(xn2), L.ptr(T1), L.ptr(T2), L.ptr(got)) == 1
        if st == 1 and r["status"] == 1:
            assert np.array_equal(got.view(np.uint32), r["x3D"].view(np.uint32))   # the record's point is this one
        scale = np.linalg.norm(want)
        ours = max(ours, float(np.linalg.norm(got - want) / scale))
        lapack32 = max(lapack32, float(np.linalg.norm(lapack_x3D(A, f32) - want) / scale))
        n_tri += 1
    return ours, lapack32, close, flipped, n_tri


def test_svd_accuracy_and_every_status_against_a_float64_model(emu_lib):
    """On the golden main case (tests/golden/new_points/main.json: the reference's pose arithmetic, the far-point threshold kept in
    the fixture), every match reported: the relative error of x3D of the triangulated matches against a float64 LAPACK SVD of the
    same fp32 A stays within 4 x what numpy.linalg.svd in float32 reaches on the same matrices (an independent SVD; the factor
    covers two correct implementations differing by a small constant).  Both maxima are the ones the fixture records:
    9.55e-08 for both on 271 triangulated matches - numpy's float32 SVD returns the correctly rounded float64 result here, which
    is why np_triangulate sweeps in fp64.  Every status equals the float64 model's, except for matches where some float64
    comparison has a relative margin below 1e-3 (on 1 - cos for the parallax ones) - at most 2 % of the fixture: 2 of 680."""
    import new_points_golden as ng
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    case, fx = ng.fixture_case("main")
    recs = mt.CreateNewMapPointsRestatement(nc.oracle_search, case["kf1"], case["neighbours"], dict(case["prm"], report_rejected=1), case["skip"])[0]
    mt.close()
    ours, lapack32, close, flipped, n_tri = svd_maxima(emu_lib, case, recs)
    print("triangulated %d: max relative error of x3D %.3g (np_triangulate), %.3g (numpy.linalg.svd in float32); %d of %d within the margin"
          % (n_tri, ours, lapack32, close, len(recs)))
    assert n_tri >= 200
    assert ours <= 4 * lapack32, (ours, lapack32)
    assert close <= 0.02 * len(recs), (close, len(recs))
    assert not flipped, flipped[:5]
    svd = fx["svd"]
    assert (svd["triangulated"], svd["records"], svd["within_margin"]) == (n_tri, len(recs), close)
    assert svd["max_rel_error_np_triangulate"] == ours and svd["max_rel_error_numpy_float32_svd"] == lapack32
