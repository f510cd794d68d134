"""The golden isInFrustum cases.  tests/golden/frustum/*.json hold, for up to 256 points of a generated local map, what the
reference's OWN Frame::isInFrustum + MapPoint::PredictScale left in the MapPoint (result bits), next to the generator
parameters:

    python tests/frustum_golden.py         # rewrites the fixtures (needs the reference sources)

The reference's functions are cut out of its sources by signature at test time (tests/_build/frustum_ref_bodies.inc, never
committed) and compiled unmodified against tests/frustum_ref_types.h (tests/frustum_ref_glue.cpp).  Three back ends produce
a case's results: that code, the numpy restatement (F.frustum_restatement) and the device library."""
import ctypes as C
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

import frustum_edges  # noqa: E402
from orb_slam3_rgbl_amd import _lib as L  # noqa: E402
from orb_slam3_rgbl_amd import cases  # noqa: E402
from orb_slam3_rgbl_amd import frontend as F  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "frustum")
REF = "/root/reference"
MAX_POINTS = 256

CASES = {
    "kitti": dict(n1=600, n2=500, seed=71),
    "second": dict(n1=600, n2=500, seed=72),
    "third": dict(n1=500, n2=300, seed=73),
}

# (file, the definition's first line as a regular expression)
SIGNATURES = [
    ("src/Frame.cc", r"bool\s+Frame::isInFrustum\s*\(\s*MapPoint\s*\*\s*pMP\s*,\s*float\s+viewingCosLimit\s*\)"),
    ("src/MapPoint.cc", r"int\s+MapPoint::PredictScale\s*\(\s*const\s+float\s*&\s*currentDist\s*,\s*Frame\s*\*\s*pF\s*\)"),
    ("src/MapPoint.cc", r"float\s+MapPoint::GetMinDistanceInvariance\s*\(\s*\)"),
    ("src/MapPoint.cc", r"float\s+MapPoint::GetMaxDistanceInvariance\s*\(\s*\)"),
    ("src/CameraModels/Pinhole.cpp", r"Eigen::Vector2f\s+Pinhole::project\s*\(\s*const\s+Eigen::Vector3f\s*&\s*v3D\s*\)"),
]


def have_reference():
    return all(os.path.exists(os.path.join(REF, f)) for f, _ in SIGNATURES)


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


def build_reference_glue():
    out = os.path.join(TESTS, "_build", "libref_frustum.so")
    inc = os.path.join(TESTS, "_build", "frustum_ref_bodies.inc")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    bodies = "\n\n".join(cut_function(open(os.path.join(REF, f), errors="replace").read(), sig) for f, sig in SIGNATURES) + "\n"
    if not os.path.exists(inc) or open(inc).read() != bodies:
        with open(inc, "w") as f:
            f.write(bodies)
    deps = [inc, os.path.join(TESTS, "frustum_ref_glue.cpp"), os.path.join(TESTS, "frustum_ref_types.h"),
            os.path.join(ROOT, "oracle", "cvcompat", "sophus", "sim3.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        tmp = out + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w", "-shared", "-o", tmp,
                               "-I" + TESTS, "-I" + os.path.dirname(inc), "-I" + os.path.join(ROOT, "oracle", "cvcompat"),
                               os.path.join(TESTS, "frustum_ref_glue.cpp")])
        os.replace(tmp, out)
    lib = C.CDLL(out)
    V, I, Fl = C.c_void_p, C.c_int, C.c_float
    lib.ref_frustum.restype = None
    lib.ref_frustum.argtypes = [I, V, V, V, V, V, V, V, V, V, V, Fl, Fl, I, Fl, V, V, V, V]
    return lib


def make_case(name=None, **params):
    """the generated local map with its edge points, and which points the fixture records"""
    p = params or CASES[name]
    c, named = frustum_edges.add_frustum_edge_points(cases.make_local_map_case(p["n1"], p["n2"], p["seed"]))
    rest = np.setdiff1d(np.arange(p["n1"]), list(named.values()))
    c["consider1"][np.random.default_rng(p["seed"]).choice(rest, p["n1"] // 12, replace=False)] = 0
    pick = sorted(named.values()) + [int(i) for i in rest[:MAX_POINTS - len(named)]]
    return c, named, np.array(sorted(pick[:MAX_POINTS]))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def reference_results(case, lib=None):
    """(in_view, records) from the reference's own code.  Fields the reference leaves unwritten are reported as the restatement
    and the device report them: 0 (proj_xr, depth, view_cos, level of a point that is not in view), (-1, -1) (the projection of a
    point that is not considered)."""
    lib = lib or build_reference_glue()
    n1 = len(case["world_pos1"])
    a = {k: np.ascontiguousarray(case[k], np.float32) for k in ("world_pos1", "normal1", "min_dist1", "max_dist1", "Rcw", "tcw", "Ow", "K")}
    cons = None if case.get("consider1") is None else np.ascontiguousarray(case["consider1"], np.uint8)
    bounds = np.ascontiguousarray(np.asarray(case["grid"], np.float32)[:4])
    iv, ret, rec5, level = np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros((n1, 5), np.float32), np.zeros(n1, np.int32)
    lib.ref_frustum(n1, _p(cons), _p(a["world_pos1"]), _p(a["normal1"]), _p(a["min_dist1"]), _p(a["max_dist1"]), _p(a["Rcw"]), _p(a["tcw"]),
                    _p(a["Ow"]), _p(a["K"]), _p(bounds), float(case["mbf"]), float(case["log_scale_factor"]),
                    int(case.get("n_levels", len(case["scale_factors"]))), float(case["viewing_cos_limit"]), _p(iv), _p(ret), _p(rec5), _p(level))
    assert np.array_equal(iv, ret)                       # the return value is mbTrackInView
    considered = np.ones(n1, bool) if cons is None else cons != 0
    out_of_view = considered & (iv == 0)
    assert (rec5[out_of_view, 2:] == -7).all() and (level[out_of_view] == -7).all()   # ... and those four stay as they were
    assert (rec5[~considered] == -7).all()
    rec = np.zeros(n1, L.FRUSTUM_DTYPE)
    seen = iv != 0
    rec["proj_x"], rec["proj_y"] = np.where(considered, rec5[:, 0], -1), np.where(considered, rec5[:, 1], -1)
    for k, fld in ((2, "proj_xr"), (3, "depth"), (4, "view_cos")):
        rec[fld] = np.where(seen, rec5[:, k], 0)
    rec["level"] = np.where(seen, level, 0)
    return iv, rec


def restatement_results(case):
    iv, rec, _ = F.frustum_restatement(case)
    return iv, rec


def device_results(lib):
    def run(case):
        mt = F.ORBmatcher(0.8, True, lib=lib)
        iv, rec, _ = mt.FrustumCull(case)
        mt.close()
        return iv, rec
    return run


FIELDS = ("proj_x", "proj_y", "proj_xr", "depth", "view_cos")


def canonical(a):
    """float32 bits with every NaN as one NaN"""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32)).astype(np.uint32)


def encode(iv, rec, pick):
    d = dict(index=[int(i) for i in pick], in_view="".join(str(int(v)) for v in iv[pick]), level="".join("%x" % int(v) for v in rec["level"][pick]))
    for fld in FIELDS:
        d[fld] = "".join("%08x" % int(v) for v in canonical(rec[fld][pick]))
    return d


def check_conditions(case, named, pick, iv, rec):
    """What every fixture has to contain, on the recorded results (the rejecting test of a point is the restatement's, whose
    results equal the recorded ones)."""
    wiv, wrec, stage = F.frustum_restatement(case)
    assert encode(wiv, wrec, pick) == encode(iv, rec, pick)
    st = stage[pick]
    share = {s: float((st == s).mean()) for s in range(6)}
    assert all(share[s] >= 0.05 for s in (1, 2, 3, 4, 5)) and share[5] >= 0.30, share
    n_levels = len(case["scale_factors"])
    seen = pick[iv[pick] != 0]
    assert set(int(v) for v in rec["level"][seen]) == set(range(n_levels))
    raw = frustum_edges.predict_scale_unclamped(F.frustum_terms(case)["ratio"][seen], case["log_scale_factor"])
    assert (raw < 0).any() and (raw >= n_levels).any(), "both clamps of PredictScale"
    # the edge points are where they were put
    T = F.frustum_terms(case)
    g = np.asarray(case["grid"], np.float32)
    assert T["u"][named["u_min"]] == g[0] and T["u"][named["u_max"]] == g[2] and T["v"][named["v_min"]] == g[1] and T["v"][named["v_max"]] == g[3]
    assert all(iv[named[k]] for k in ("u_min", "u_max", "v_min", "v_max", "dist_min_on", "dist_max_on", "view_cos_on"))
    assert not any(iv[named[k]] for k in ("dist_min_out", "dist_max_out", "view_cos_below", "zero_depth"))
    assert T["z"][named["zero_depth"]] == 0 and T["x"][named["zero_depth"]] != 0
    assert T["view_cos"][named["view_cos_on"]] == np.float32(case["viewing_cos_limit"])
    assert T["dist"][named["dist_min_on"]] == np.float32(0.8) * case["min_dist1"][named["dist_min_on"]]
    assert T["dist"][named["dist_max_on"]] == np.float32(1.2) * case["max_dist1"][named["dist_max_on"]]
    sf = np.asarray(case["scale_factors"], np.float32)
    for lv in range(1, n_levels):
        on, below, above = (named["ratio_%d_%s" % (lv, w)] for w in ("on", "below", "above"))
        assert T["ratio"][on] == sf[lv] and T["ratio"][below] < sf[lv] < T["ratio"][above]
        assert np.nextafter(T["ratio"][below], np.float32(9)) == sf[lv] == np.nextafter(T["ratio"][above], np.float32(0))
    assert set(named.values()) <= set(int(i) for i in pick)


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def assert_matches_golden(name, backend):
    """runs the case on `backend` (case -> (in_view, records)) and compares with the fixture; returns the points in view"""
    want = load(name)
    assert want["params"] == CASES[name]
    case, named, pick = make_case(name)
    iv, rec = backend(case)
    got = encode(iv, rec, pick)
    for key in ("index", "in_view", "level") + FIELDS:
        assert got[key] == want["results"][key], "%s: %s differs from the fixture" % (name, key)
    return int(iv[pick].sum())


def main():
    lib = build_reference_glue()
    os.makedirs(GOLDEN, exist_ok=True)
    for name, params in CASES.items():
        case, named, pick = make_case(name)
        iv, rec = reference_results(case, lib)
        check_conditions(case, named, pick, iv, rec)
        path = os.path.join(GOLDEN, name + ".json")
        with open(path, "w") as f:
            json.dump(dict(params=params, results=encode(iv, rec, pick)), f, separators=(",", ":"))
            f.write("\n")
        assert os.path.getsize(path) <= 16 * 1024, path
        print("%s: %d points, %d in view, %d bytes" % (name, len(pick), int(iv[pick].sum()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
