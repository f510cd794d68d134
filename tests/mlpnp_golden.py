"""The golden MLPnPsolver runs.  tests/golden/mlpnp/<case>.json hold what the reference's OWN constructor, iterate,
SetRansacParameters, CheckInliers and Refine (src/MLPnPsolver.cpp) and Pinhole::project / unproject did on a generated case after
srand(seed): mRansacMinInliers, mRansacMaxIts and N, and for every call of iterate(5, ...) the sets it drew, the return value,
bNoMore, nInliers, mnIterations and mnBestInliers after the call, the bits of Tout and of mBestTcw, and vbInliers.

    python tests/mlpnp_golden.py         # rewrites the fixtures (needs the reference sources)

The definitions are cut out of the reference by signature at test time (sim3_golden.cut_function) into
tests/_build/mlpnp_ref_bodies.inc (never committed) and compiled unmodified against tests/mlpnp_ref_types.h
(tests/mlpnp_ref_glue.cpp); DUtils::Random is the reference's own Thirdparty/DBoW2/DUtils/Random.cpp over rand().  There is no
Eigen on the build machine, so computePose itself cannot be compiled: the stand-in forwards a six-point call to the host build of
csrc/mlpnp_math.h and answers Refine's call with NaN.  This pins the constructor's bookkeeping, SetRansacParameters, the sampling
order, the `||` of the loop condition, the `>=` and `>` rules, what Refine returns AS COMPILED (the current hypothesis: the pose
it computes is never read - the NaN of the stand-in shows up nowhere), the mapping through mvKeyPointIndices and the
N < mRansacMinInliers exit.  It does NOT pin computePose: that is the model's (tests/mlpnp_model.py).
A case's inputs are regenerated from the parameters in its fixture."""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p_ in (ROOT, TESTS):
    if _p_ not in sys.path:
        sys.path.insert(0, _p_)

from orb_slam3_rgbl_amd import mlpnp_cases as mc  # noqa: E402
from sim3_golden import cut_function, hexbits, hexf  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "mlpnp")
BUILD = os.path.join(TESTS, "_build")
REF = "/root/reference"
DUTILS = os.path.join(REF, "Thirdparty", "DBoW2", "DUtils")
SOLVER = "src/MLPnPsolver.cpp"
PINHOLE = "src/CameraModels/Pinhole.cpp"
SIGNATURES = [(SOLVER, r"MLPnPsolver::MLPnPsolver\s*\(\s*const\s+Frame\s*&\s*F[^)]*\)\s*:[^{]*"),
              (SOLVER, r"bool\s+MLPnPsolver::iterate\s*\([^)]*\)"),
              (SOLVER, r"void\s+MLPnPsolver::SetRansacParameters\s*\([^)]*\)"),
              (SOLVER, r"void\s+MLPnPsolver::CheckInliers\s*\(\s*\)"),
              (SOLVER, r"bool\s+MLPnPsolver::Refine\s*\(\s*\)"),
              (PINHOLE, r"cv::Point2f\s+Pinhole::project\s*\(\s*const\s+cv::Point3f\s*&\s*p3D\s*\)"),
              (PINHOLE, r"cv::Point3f\s+Pinhole::unproject\s*\(\s*const\s+cv::Point2f\s*&\s*p2D\s*\)")]
STEP = 5   # Tracking.cc:3713: iterate(5, ...)

# (the numbers in test_mlpnp_reference.test_fixture_conditions)
CASES = {
    "first_qualifying": dict(seed=0, N=60, min_inliers=10, outlier_share=0.3, pixel_noise=0.3, after_success=0),
    "failed_refine": dict(seed=17, N=20, min_inliers=10, outlier_share=0.3, pixel_noise=0.3, after_success=0),
    "best_after_run_through": dict(seed=1, N=20, min_inliers=10, outlier_share=0.5, pixel_noise=0.0, after_success=0),
    "runs_through": dict(seed=5, N=40, min_inliers=10, outlier_share=1.0, pixel_noise=0.3, after_success=0),
    "too_few": dict(seed=6, N=9, min_inliers=10, outlier_share=0.3, pixel_noise=0.3, after_success=0),
    "min_equals_n": dict(seed=7, N=12, min_inliers=12, outlier_share=0.0, pixel_noise=0.0, after_success=0),
    "second_call": dict(seed=2, N=60, min_inliers=10, outlier_share=0.3, pixel_noise=0.3, after_success=1),
}


def have_reference():
    return all(os.path.exists(os.path.join(REF, f)) for f in (SOLVER, PINHOLE)) and os.path.exists(os.path.join(DUTILS, "Random.cpp"))


def ref_case(seed, N, min_inliers, outlier_share, pixel_noise, after_success):
    """a generator case as the constructor sees it: features without a map point and with a bad one in between"""
    case = mc.make_mlpnp_case(N, 0, seed=seed + 500, outlier_share=outlier_share, pixel_noise=pixel_noise)
    rng = np.random.default_rng(seed + 1500)
    n = len(case["mp_index"])
    state = (case["mp_index"] >= 0).astype(np.int32)
    free = np.nonzero(state == 0)[0]
    state[free[rng.random(len(free)) < 0.4]] = 2                      # a bad map point: skipped (:70)
    wp = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
    has = case["mp_index"] >= 0
    wp[has] = case["world_pos"][case["mp_index"][has]]
    mn, max_its = mc.ransac_parameters(N, min_inliers=min_inliers)
    pr = mc.problem(case, min_inliers=mn)
    return dict(seed=seed, n=n, state=state, wp=wp, case=case, pr=pr, min_inliers=min_inliers, mn=mn, max_its=max_its, after_success=after_success)


def write_case(c, path):
    case = c["case"]
    with open(path, "wb") as f:
        f.write(struct.pack("<ifiiiff", c["seed"], 0.99, c["min_inliers"], 300, 6, 0.5, 5.991))
        f.write(struct.pack("<5i", STEP, 400, c["after_success"], c["n"], len(case["level_sigma2"])))
        for a, dt in ((c["state"], np.int32), (case["octave"], np.int32), (case["xy"], np.float32), (c["wp"], np.float32), (case["K"], np.float32),
                      (case["level_sigma2"], np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def build_reference():
    """tests/_build/mlpnp_ref: the reference's definitions and DUtils::Random behind tests/mlpnp_ref_glue.cpp"""
    exe, inc = os.path.join(BUILD, "mlpnp_ref"), os.path.join(BUILD, "mlpnp_ref_bodies.inc")
    os.makedirs(BUILD, exist_ok=True)
    text = {f: open(os.path.join(REF, f), errors="replace").read() for f in (SOLVER, PINHOLE)}
    bodies = "namespace ORB_SLAM3 {\n" + "\n\n".join(cut_function(text[f], sig) for f, sig in SIGNATURES) + "\n}\n"
    assert not re.search(r"#\s*include", bodies)
    if not os.path.exists(inc) or open(inc).read() != bodies:
        with open(inc, "w") as f:
            f.write(bodies)
    glue = os.path.join(TESTS, "mlpnp_ref_glue.cpp")
    deps = [inc, glue, os.path.join(TESTS, "mlpnp_ref_types.h"), os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc", "mlpnp_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w", "-o", tmp, "-I" + TESTS, "-I" + BUILD,
                               "-I" + os.path.dirname(DUTILS), "-I" + DUTILS, glue, os.path.join(DUTILS, "Random.cpp"), os.path.join(DUTILS, "Timestamp.cpp")])
        os.replace(tmp, exe)
    return exe


def parse_reference(buf, n):
    mn, max_its, N, n_calls = struct.unpack_from("<4i", buf)
    off = 16
    calls = []
    for _ in range(n_calls):
        ran, ret, no_more, inliers, iterations, best = struct.unpack_from("<6i", buf, off)
        off += 24
        sets = np.frombuffer(buf, np.int32, 6 * ran, off)
        off += 24 * ran
        T, B = np.frombuffer(buf, np.float32, 16, off), np.frombuffer(buf, np.float32, 16, off + 64)
        off += 128
        flags = np.frombuffer(buf, np.uint8, n, off)
        off += n
        # Eigen::Matrix4f is column-major; the stand-in's d[i][j] is row-major: recorded row-major
        calls.append(dict(ran=ran, ret=ret, no_more=no_more, inliers=inliers, iterations=iterations, best=best, sets=[int(v) for v in sets],
                          T=hexf(T), best_Tcw=hexf(B), flags=hexbits(flags)))
    six, other = struct.unpack_from("<2i", buf, off)
    assert off + 8 == len(buf)
    return dict(min_inliers=mn, max_its=max_its, N=N, calls=calls, six_point_poses=six, refine_poses=other)


def reference_run(exe, params):
    c = ref_case(**params)
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
        write_case(c, path)
        res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "MLPNP_REF_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
        return dict(params=dict(params), **parse_reference(open(out, "rb").read(), c["n"]))


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


IDENTITY = hexf(np.eye(4, dtype=np.float32))
ZERO = hexf(np.zeros(16, np.float32))


def check_against_host_build(fx, lib):
    """every recorded call against rgbl_mlpnp_ransac_host on the sets the reference drew, the state carried from call to call:
    the scan stops where the reference's loop stopped, with the same return value, bNoMore, nInliers, matrix bits, mBestTcw bits,
    mnBestInliers and the same flags through mvKeyPointIndices.  Returns the per-hypothesis counts of every call."""
    from orb_slam3_rgbl_amd import frontend as F
    c = ref_case(**fx["params"])
    N, n = c["case"]["N"], c["n"]
    assert (fx["N"], fx["min_inliers"]) == (N, c["mn"]) and (N < c["mn"] or fx["max_its"] == c["max_its"])   # the constructor's count, SetRansacParameters
    none = hexbits(np.zeros(n, np.uint8))
    state = dict(best_inliers=0, best_mask=None, best_Tcw=np.zeros((4, 4), np.float32))   # a fresh stand-in matrix is zero
    iterations, counts = 0, []
    for k, call in enumerate(fx["calls"]):
        if N < c["mn"]:   # :106-110
            assert (call["ran"], call["ret"], call["no_more"], call["inliers"], call["iterations"], call["best"]) == (0, 0, 1, 0, 0, 0)
            assert call["T"] == IDENTITY and call["flags"] == none and len(fx["calls"]) == 1
            res = F.mlpnp_ransac_host(dict(c["pr"], samples=None, n_hyp=STEP), lib)
            assert (res["found"], res["no_more"], res["n_inliers"], res["iterations_run"]) == (0, 1, 0, 0) and hexf(res["Tcw"]) == IDENTITY
            continue
        if not call["ret"]:
            assert call["ran"] == mc.calls_n_hyp(fx["max_its"], iterations, STEP), k          # the `||` of :115
        samples = np.array(call["sets"], np.int32).reshape(call["ran"], 6)
        res = F.mlpnp_ransac_host(dict(c["pr"], samples=samples, n_hyp=call["ran"], **state), lib)
        counts.append(res["counts"])
        iterations += call["ran"]
        assert (res["iterations_run"], res["found"], res["no_more"], res["n_inliers"]) == (call["ran"], call["ret"], call["no_more"], call["inliers"]), (k, res["iterations_run"], res["found"])
        assert (call["iterations"], call["best"]) == (iterations, res["best_inliers"]), k
        assert call["T"] == hexf(res["Tcw"]) and call["best_Tcw"] == hexf(res["best_Tcw"]), k
        assert call["flags"] == (hexbits(res["inlier"]) if call["ret"] else none), k
        state = dict(best_inliers=res["best_inliers"], best_mask=res["best_mask"][:N] if res["best_inliers"] else None, best_Tcw=res["best_Tcw"])
    return counts


def main():
    exe = build_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    for name, params in CASES.items():
        fx = reference_run(exe, params)
        path = os.path.join(GOLDEN, name + ".json")
        with open(path, "w") as f:
            json.dump(fx, f, separators=(",", ":"))
            f.write("\n")
        assert os.path.getsize(path) <= 16 * 1024, (path, os.path.getsize(path))
        print("%s: min %d, max_its %d, N %d, %s, poses %d + %d, %d bytes" % (name, fx["min_inliers"], fx["max_its"], fx["N"],
              [(c["ran"], c["ret"], c["no_more"], c["inliers"], c["best"]) for c in fx["calls"]], fx["six_point_poses"], fx["refine_poses"],
              os.path.getsize(path)))


def build_shim(lib_path, tag):
    """tests/_build/mlpnp_shim_<tag>: the drop-in rgbl_shim::MLPnPsolver behind the same glue (-DMLPNP_SHIM), linked with lib_path.
    Nothing of the reference is needed: the glue brings its own DUtils::Random stand-in and camera."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "mlpnp_shim_" + tag)
    glue = os.path.join(TESTS, "mlpnp_ref_glue.cpp")
    deps = [glue, os.path.join(TESTS, "mlpnp_ref_types.h"), os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim", "MLPnPsolver.h"),
            os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc", "mlpnp_math.h"), lib_path]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                               "-DMLPNP_SHIM", "-o", tmp, "-I" + TESTS, "-I" + os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim"),
                               "-I" + os.path.join(ROOT, "include"), glue, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)])
        os.replace(tmp, exe)
    return exe


def shim_run(exe, params):
    c = ref_case(**params)
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
        write_case(c, path)
        res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "MLPNP_REF_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
        return parse_reference(open(out, "rb").read(), c["n"])


def check_shim_against_fixture(got, fx):
    """the drop-in's calls against the recorded ones, up to and including the first success: from there on the drop-in's random
    stream is further along than the reference's (the documented deviation).  mBestTcw is compared once a hypothesis is held
    (before that it is the identity here and uninitialised in the reference).  Returns the number of calls compared."""
    assert (got["min_inliers"], got["N"]) == (fx["min_inliers"], fx["N"]) and (fx["N"] < fx["min_inliers"] or got["max_its"] == fx["max_its"])
    n = 0
    for a, b in zip(got["calls"], fx["calls"]):
        for key in ("ran", "ret", "no_more", "inliers", "iterations", "best", "sets", "T", "flags") + (("best_Tcw",) if b["best"] > 0 else ()):
            assert a[key] == b[key], (n, key, a[key], b[key])
        if b["best"] == 0:
            assert a["best_Tcw"] == IDENTITY, n
        n += 1
        if b["ret"]:
            break
    assert n >= 1 and len(got["calls"]) == len(fx["calls"])
    return n

if __name__ == "__main__":
    main()
