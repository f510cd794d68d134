"""The golden CreateNewMapPoints cases.  tests/golden/new_points/*.json hold what the reference's OWN
LocalMapping::CreateNewMapPoints left in mlpRecentAddedMapPoints - (neighbour, idx1, idx2, world position bits) of the first
RECORDED points, the count and a digest of all - next to the generator parameters and the geometry the reference's Sophus
arithmetic (the stand-in's) makes of the poses: matrix3x4() and camera centre per key frame, R12 / t12 / epipole per neighbour.

    python tests/new_points_golden.py         # rewrites the fixtures (needs the reference sources and oracle/_ref)

The reference's functions - LocalMapping::CreateNewMapPoints, GeometricTools::Triangulate, KeyFrame::UnprojectStereo,
Pinhole::unprojectEig, Pinhole::project - are cut out of its sources by signature at test time
(tests/_build/new_points_ref_bodies.inc, never committed) and compiled unmodified against tests/new_points_ref_types.h
(tests/new_points_ref_glue.cpp); SearchForTriangulation inside is the reference's own ORBmatcher.cc
(oracle/_ref/libref_orbmatcher.so).  This pins the control flow of :434-711, the overload resolution of cos / atan2 and the
order of the tests.  It does NOT pin the SVD (the JacobiSVD stand-in hands out csrc/newpoint_math.h's null vector) or Eigen's
evaluation order (the stand-in's): those stay the project's reading, as elsewhere.
Three back ends produce a case's results: that code, the restatement (frontend's, with the oracle's search) and the device."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p_ in (ROOT, TESTS):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

from oracle import oracle_py as O  # noqa: E402
from orb_slam3_rgbl_amd import _lib as L  # noqa: E402
from orb_slam3_rgbl_amd import cases  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "new_points")
REF = "/root/reference"
REF_MATCHER = os.path.join(ROOT, "oracle", "_ref", "libref_orbmatcher.so")
RECORDED = 200

CASES = {
    "main": dict(n=600, n_neigh=10, seed=7),                     # th_far_points: chosen when the fixture is written, kept in it
    "inertial": dict(n=300, n_neigh=5, seed=9, inertial=1),
    "monocular": dict(n=300, n_neigh=5, seed=9, monocular=1),
}
MEDIAN_DEPTH = {"monocular": (30.0, 200.0, 30.0, 30.0, 30.0)}     # neighbour 1: baseline / median depth < 0.01 (:455-459)

SIGNATURES = [
    ("src/LocalMapping.cc", r"void\s+LocalMapping::CreateNewMapPoints\s*\(\s*\)"),
    ("src/GeometricTools.cc", r"bool\s+GeometricTools::Triangulate\s*\(\s*Eigen::Vector3f\s*&\s*x_c1\s*,[^)]*\)"),
    ("src/KeyFrame.cc", r"bool\s+KeyFrame::UnprojectStereo\s*\(\s*int\s+i\s*,\s*Eigen::Vector3f\s*&\s*x3D\s*\)"),
    ("src/CameraModels/Pinhole.cpp", r"Eigen::Vector3f\s+Pinhole::unprojectEig\s*\(\s*const\s+cv::Point2f\s*&\s*p2D\s*\)"),
    ("src/CameraModels/Pinhole.cpp", r"cv::Point2f\s+Pinhole::project\s*\(\s*const\s+cv::Point3f\s*&\s*p3D\s*\)"),
]


def have_reference():
    return all(os.path.exists(os.path.join(REF, f)) for f, _ in SIGNATURES) and os.path.exists(REF_MATCHER)


def cut_function(text, signature):
    """the definition that starts with `signature`: up to the brace that closes its body"""
    m = re.search(signature + r"\s*\{", text)
    assert m, signature
    depth, k = 0, m.end() - 1
    while True:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
        if depth == 0:
            return text[m.start():k]


class KfArrays(C.Structure):
    _fields_ = [("n", C.c_int), ("desc", C.c_void_p), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("kp_angle", C.c_void_p),
                ("uright", C.c_void_p), ("has_mp", C.c_void_p), ("nnodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p),
                ("node_feat", C.c_void_p)]


class KfIn(C.Structure):
    _fields_ = [("a", KfArrays), ("depth", C.c_void_p), ("xy_raw", C.c_void_p), ("q", C.c_float * 4), ("t", C.c_float * 3),
                ("median_depth", C.c_float)]


def build_reference_glue():
    out = os.path.join(TESTS, "_build", "libref_new_points.so")
    inc = os.path.join(TESTS, "_build", "new_points_ref_bodies.inc")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    bodies = "\n\n".join(cut_function(open(os.path.join(REF, f), errors="replace").read(), sig) for f, sig in SIGNATURES) + "\n"
    if not os.path.exists(inc) or open(inc).read() != bodies:
        with open(inc, "w") as f:
            f.write(bodies)
    deps = [inc, os.path.join(TESTS, "new_points_ref_glue.cpp"), os.path.join(TESTS, "new_points_ref_types.h"),
            os.path.join(ROOT, "oracle", "cvcompat", "sophus", "sim3.hpp")] + \
           [os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc", h) for h in ("newpoint_math.h", "frustum_math.h", "sincos_glibc.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden", "-w", "-shared",
                               "-o", tmp, "-I" + TESTS, "-I" + os.path.dirname(inc), "-I" + os.path.join(ROOT, "oracle", "cvcompat"),
                               os.path.join(TESTS, "new_points_ref_glue.cpp"), "-ldl"])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    V, I, Fl = C.c_void_p, C.c_int, C.c_float
    lib.ref_np_open_matcher.restype, lib.ref_np_open_matcher.argtypes = I, [C.c_char_p]
    lib.ref_np_pose.restype, lib.ref_np_pose.argtypes = None, [V] * 4
    lib.ref_np_pair.restype, lib.ref_np_pair.argtypes = None, [V] * 8
    lib.ref_create_new_map_points.restype = I
    lib.ref_create_new_map_points.argtypes = [C.POINTER(KfIn), I, V, V, Fl, Fl, V, V, I, Fl, I, I, I, Fl, I, V, V]
    assert lib.ref_np_open_matcher(REF_MATCHER.encode()) == 0
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def reference_geometry(lib, case):
    """per key frame (the current one first) matrix3x4() and centre, per neighbour R12, t12, epipole - from (q, t) in fp32"""
    kfs = [case["kf1"]] + [nb["kf"] for nb in case["neighbours"]]
    K = np.ascontiguousarray(case["kf1"]["K"], np.float32)
    poses, pairs = np.zeros((len(kfs), 15), np.float32), np.zeros((len(kfs) - 1, 14), np.float32)
    qt = [(np.ascontiguousarray(kf["q"], np.float32), np.ascontiguousarray(np.asarray(kf["Tcw"], np.float32).reshape(3, 4)[:, 3])) for kf in kfs]
    for i, (q, t) in enumerate(qt):
        lib.ref_np_pose(_p(q), _p(t), _p(poses[i, :12]), _p(poses[i, 12:]))
    for i in range(1, len(kfs)):
        lib.ref_np_pair(_p(qt[0][0]), _p(qt[0][1]), _p(qt[i][0]), _p(qt[i][1]), _p(K), _p(pairs[i - 1, :9]), _p(pairs[i - 1, 9:12]), _p(pairs[i - 1, 12:]))
    return poses, pairs


def make_case(name, geometry, th_far_points=None):
    """the generated case with the reference's geometry in place of the generator's float64 one; skip[] as the reference's own
    tests give it (none, or the monocular median-depth test)"""
    p = dict(CASES[name])
    case = cases.make_new_points_case(th_far_points=th_far_points, report_rejected=0, **p)
    if geometry is None:
        return case
    poses, pairs = geometry
    kfs = [case["kf1"]] + [nb["kf"] for nb in case["neighbours"]]
    for kf, g in zip(kfs, poses):
        kf["Tcw"], kf["Ow"] = g[:12].copy(), g[12:].copy()
    K = case["kf1"]["K"]
    for nb, g in zip(case["neighbours"], pairs):
        nb["F12"], nb["ep"] = O.fundamental(K, K, g[:9], g[9:12]), g[12:].copy()
    case["skip"][:] = 0
    if name in MEDIAN_DEPTH:
        import new_points_checks as nc
        for i, nb in enumerate(case["neighbours"]):
            baseline = nc.f32_norm(np.asarray(nb["kf"]["Ow"], np.float32) - np.asarray(case["kf1"]["Ow"], np.float32))
            case["skip"][i] = (np.float32(baseline / np.float32(MEDIAN_DEPTH[name][i]))) < 0.01   # float / float, compared with a double
    return case


def reference_results(lib, name, case, prepare=False):
    """mlpRecentAddedMapPoints after the reference's own function, as accepted records (status unknown: 0); prepare=True: the
    closure that makes the call (tools/new_points_bench.py times it)"""
    keep = []

    def kfin(kf, median):
        k = KfIn()
        k.a.n = len(kf["desc"])
        for field, key, dt in (("desc", "desc", np.uint8), ("kp_xy", "xy", np.float32), ("kp_octave", "octave", np.int32),
                               ("kp_angle", "angle", np.float32), ("uright", "uright", np.float32), ("has_mp", "has_mp", np.uint8),
                               ("node_id", "node_id", np.int32), ("node_off", "node_off", np.int32), ("node_feat", "node_feat", np.int32)):
            a = np.ascontiguousarray(kf[key], dt)
            keep.append(a)
            setattr(k.a, field, a.ctypes.data)
        k.a.nnodes = len(kf["node_id"])
        for field, key in (("depth", "depth"), ("xy_raw", "xy_raw")):
            a = np.ascontiguousarray(kf[key], np.float32)
            keep.append(a)
            setattr(k, field, a.ctypes.data)
        t = np.asarray(kf["Tcw"], np.float32).reshape(3, 4)[:, 3]
        for i in range(4):
            k.q[i] = float(kf["q"][i])
        for i in range(3):
            k.t[i] = float(t[i])
        k.median_depth = float(median)
        return k
    kf1, prm = case["kf1"], case["prm"]
    nn = len(case["neighbours"])
    med = MEDIAN_DEPTH.get(name, (1.0,) * nn)
    k1 = kfin(kf1, 1.0)
    k2 = (KfIn * nn)(*[kfin(nb["kf"], med[i]) for i, nb in enumerate(case["neighbours"])])
    cap = len(kf1["desc"]) + 1
    idx, x3D = np.zeros((cap, 3), np.int32), np.zeros((cap, 3), np.float32)
    K, sf, s2 = (np.ascontiguousarray(kf1[k], np.float32) for k in ("K", "scale_factors", "level_sigma2"))
    def call(_keep=keep):
        n = lib.ref_create_new_map_points(C.byref(k1), nn, C.cast(k2, C.c_void_p), _p(K), float(kf1["mb"]), float(kf1["mbf"]), _p(sf), _p(s2), len(sf),
                                          1.2, int(prm["monocular"]), int(prm["inertial"]), int(prm["far_points"]), float(prm["th_far_points"]),
                                          cap, _p(idx), _p(x3D))
        assert 0 <= n <= cap, n
        rec = np.zeros(n, L.NEW_POINT_DTYPE)
        rec["neighbour"], rec["idx1"], rec["idx2"], rec["x3D"] = idx[:n, 0], idx[:n, 1], idx[:n, 2], x3D[:n]
        return rec
    return call if prepare else call()


def encode(rec):
    """what a fixture records of a list of accepted records (the status is not part of it: the reference keeps none)"""
    body = np.zeros(len(rec), np.dtype([("i", "<i4", (3,)), ("x", "<u4", (3,))]))
    body["i"][:, 0], body["i"][:, 1], body["i"][:, 2] = rec["neighbour"], rec["idx1"], rec["idx2"]
    x = np.ascontiguousarray(rec["x3D"], np.float32)
    body["x"] = np.where(np.isnan(x), np.uint32(0x7fc00000), x.view(np.uint32))
    head = body[:RECORDED]
    return dict(count=len(rec), sha256=hashlib.sha256(body.tobytes()).hexdigest(),
                first="".join("%x%03x%03x%08x%08x%08x" % (r["i"][0], r["i"][1], r["i"][2], r["x"][0], r["x"][1], r["x"][2]) for r in head))


def hexf(a):
    return "".join("%08x" % int(v) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def unhex(s, shape):
    return np.array([int(s[i:i + 8], 16) for i in range(0, len(s), 8)], np.uint32).view(np.float32).reshape(shape)


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def fixture_case(name):
    """(case, fixture) from the committed fixture alone: no reference needed"""
    fx = load(name)
    assert fx["params"] == CASES[name]
    nn = CASES[name]["n_neigh"]
    geometry = (unhex(fx["poses"], (nn + 1, 15)), unhex(fx["pairs"], (nn, 14)))
    th = fx.get("th_far_points")
    return make_case(name, geometry, None if th is None else float(np.float32(float.fromhex(th)))), fx


def assert_matches_golden(name, backend):
    """runs the fixture's case on `backend` (case -> accepted records) and compares with the fixture; returns the count"""
    case, fx = fixture_case(name)
    got = encode(backend(case))
    for key in ("count", "sha256", "first"):
        assert got[key] == fx["results"][key], "%s: %s differs from the fixture" % (name, key)
    return got["count"]


def restatement_backend(mt):
    import new_points_checks as nc

    def run(case):
        return mt.CreateNewMapPointsRestatement(nc.oracle_search, case["kf1"], case["neighbours"], dict(case["prm"], report_rejected=0), case["skip"])[0]
    return run


def device_backend(mt):
    def run(case):
        return mt.CreateNewMapPoints(case["kf1"], case["neighbours"], dict(case["prm"], report_rejected=0), case["skip"])[0]
    return run


def main():
    import new_points_checks as nc
    import test_new_points_math as tm
    from orb_slam3_rgbl_amd import frontend as F
    lib = build_reference_glue()
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc"), "emu"])
    emu = L.bind(os.path.join(TESTS, "_build", "librgbl_frontend_emu.so"))
    mt = F.ORBmatcher(0.6, False, lib=emu)
    os.makedirs(GOLDEN, exist_ok=True)
    for name, params in CASES.items():
        geometry = reference_geometry(lib, make_case(name, None))
        th = None
        if name == "main":   # a far-point threshold that EQUALS the dist1 of one accepted match
            plain = make_case(name, geometry)
            acc = restatement_backend(mt)(plain)
            Ow1 = np.asarray(plain["kf1"]["Ow"], np.float32)
            d1 = np.sort(np.array([nc.f32_norm(r["x3D"] - Ow1) for r in acc], np.float32))
            th = np.float32(d1[int(0.95 * len(d1))])
        case = make_case(name, geometry, None if th is None else float(th))
        rec = reference_results(lib, name, case)
        want = restatement_backend(mt)(case)
        assert encode(want) == encode(rec), "%s: the restatement differs from the reference" % name
        fx = dict(params=params, poses=hexf(geometry[0]), pairs=hexf(geometry[1]), results=encode(rec))
        if th is not None:
            fx["th_far_points"] = float(th).hex()
            full = mt.CreateNewMapPointsRestatement(nc.oracle_search, case["kf1"], case["neighbours"], dict(case["prm"], report_rejected=1), case["skip"])[0]
            ours, lapack32, close, flipped, n_tri = tm.svd_maxima(emu, case, full)
            fx["svd"] = dict(triangulated=n_tri, max_rel_error_np_triangulate=ours, max_rel_error_numpy_float32_svd=lapack32,
                             within_margin=close, records=len(full))
        path = os.path.join(GOLDEN, name + ".json")
        with open(path, "w") as f:
            json.dump(fx, f, separators=(",", ":"))
            f.write("\n")
        assert os.path.getsize(path) <= 16 * 1024, (path, os.path.getsize(path))
        print("%s: %d new points, %d bytes" % (name, len(rec), os.path.getsize(path)))
    mt.close()


if __name__ == "__main__":
    main()
