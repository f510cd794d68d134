"""The golden OptimizeSim3 runs.  tests/golden/sim3_opt/<case>.json hold what the reference's OWN lines src/Optimizer.cc:2115-2381
did on a generated case: the return value, the number of edge pairs the set-up loop made, every optimize() call (iterations asked
for, pairs in the graph, edges with a kernel, iterations run), g2oS12 afterwards, whether mAcumHessian was zeroed, which entries of
vpMatches1 are null afterwards, and per pair obs2 and the information of its inverse edge.

    python tests/sim3_opt_golden.py         # rewrites the fixtures (needs the reference sources)

The lines are copied at test time into tests/_build/sim3_opt_ref_body.inc (never committed) and compiled unmodified against
tests/sim3_opt_ref_types.h (tests/sim3_opt_ref_glue.cpp).  This pins the set-up loop, obs2 and its level (octave 0 for a match
that is not observed in key frame 2: cv::KeyPoint has OpenCV's constructor), which pairs are dropped, nMoreIterations, the early
return and the final loop.  It does NOT pin g2o's arithmetic: the stand-in SparseOptimizer hands the graph to
csrc/sim3opt_math.h's Levenberg (tests/sim3_opt_ref_types.h).  A case's inputs are regenerated from the parameters in its
fixture; rgbl_optimize_sim3_host reproduces every fixture bit for bit with track_level2 = 0, which is what the C++ drop-in passes.
mnTrackScaleLevel itself is -1 in every case (Frame.cc:668): the reference never uses it as an index."""
import json
import os
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

from orb_slam3_rgbl_amd import sim3_cases as sc  # noqa: E402

GOLDEN = os.path.join(TESTS, "golden", "sim3_opt")
BUILD = os.path.join(TESTS, "_build")
REF = "/root/reference"
SOURCE, FIRST, LAST = "src/Optimizer.cc", 2115, 2381

# generator parameters, and how many matches are moved 60 px in image 1 afterwards
CASES = {
    "all_points": dict(n=300, matched=180, seed=3, out_kf2_share=0.15, all_points=True, bad_share=0.05, null_mp1_share=0.05, displace=0),
    "not_all_points": dict(n=300, matched=180, seed=3, out_kf2_share=0.15, bad_share=0.05, null_mp1_share=0.05, displace=0),
    "fix_scale": dict(n=200, matched=120, seed=4, fix_scale=True, displace=0),
    "nine_survive": dict(n=30, matched=12, seed=3, outlier_share=0.0, displace=3),
    "ten_survive": dict(n=30, matched=12, seed=3, outlier_share=0.0, displace=2),
    "ten_iterations": dict(n=40, matched=14, seed=13, depth=(40.0, 60.0), trans_noise=0.5, scale_noise=0.1, displace=0),
    "none_dropped": dict(n=40, matched=30, seed=75, th2=1e6, depth=(40.0, 60.0), outlier_share=0.0, rot_noise=(0.3, 0.6), trans_noise=2.0,
                         scale_noise=0.3, displace=0),
    "depth": dict(n=90, matched=60, seed=17, all_points=True, identity_poses=True, n_behind=3, n_on_plane=2, out_kf2_share=0.2, displace=0),
    "no_edge": dict(n=40, matched=30, seed=5, null_mp1_share=1.0, displace=0),
}


def have_reference():
    return os.path.exists(os.path.join(REF, SOURCE))


def make_case(params):
    p = {k: (tuple(v) if isinstance(v, list) else v) for k, v in params.items()}
    displace = p.pop("displace")
    n, matched = p.pop("n"), p.pop("matched")
    case = sc.make_sim3_opt_case(n, matched, **p)
    feat = np.nonzero(case["match_index"] >= 0)[0]
    case["xy1"][feat[1:1 + displace], 0] += np.float32(60.0)
    return case


def build_reference():
    """tests/_build/sim3_opt_ref: the reference's lines behind tests/sim3_opt_ref_glue.cpp"""
    exe, inc = os.path.join(BUILD, "sim3_opt_ref"), os.path.join(BUILD, "sim3_opt_ref_body.inc")
    os.makedirs(BUILD, exist_ok=True)
    lines = open(os.path.join(REF, SOURCE), errors="replace").read().splitlines(True)
    body = "".join(lines[FIRST - 1:LAST])
    assert body.startswith("int Optimizer::OptimizeSim3(") and body.rstrip().endswith("}"), body[:80]
    if not os.path.exists(inc) or open(inc).read() != body:
        with open(inc, "w") as f:
            f.write(body)
    glue = os.path.join(TESTS, "sim3_opt_ref_glue.cpp")
    csrc = os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc")
    deps = [inc, glue, os.path.join(TESTS, "sim3_opt_ref_types.h")] + [os.path.join(csrc, h) for h in ("sim3opt_math.h", "poseopt_math.h", "sim3_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-w", "-o", tmp, "-I" + TESTS, "-I" + BUILD, glue])
        os.replace(tmp, exe)
    return exe


def hex64(a):
    return np.ascontiguousarray(a, np.float64).tobytes().hex()


def hex32(a):
    u = np.ascontiguousarray(a, np.float32).reshape(-1)
    u = np.where(np.isnan(u), np.uint32(0x7fc00000), u.view(np.uint32))
    return "".join("%08x" % int(v) for v in u)


def reference_run(exe, params):
    """what the reference's own lines do on the case of `params`, in the fixtures' form"""
    import test_sim3_opt_shim as shim
    case = make_case(params)
    case["track_level2"] = np.full(len(case["match_index"]), -1, np.int32)
    n = len(case["match_index"])
    with tempfile.TemporaryDirectory() as tmp:
        path, out = os.path.join(tmp, "case.bin"), os.path.join(tmp, "out.bin")
        shim.write_case(case, path)
        res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "SIM3_OPT_REF_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
        buf = open(out, "rb").read()
    result, pairs, n_calls = struct.unpack_from("<3i", buf)
    off = 12
    calls = [list(struct.unpack_from("<4i", buf, off + 16 * k)) for k in range(n_calls)]
    off += 16 * n_calls
    est = np.frombuffer(buf, np.float64, 9, off)
    off += 72
    null_now = np.frombuffer(buf, np.uint8, n, off)
    off += n
    e21 = np.frombuffer(buf, np.float32, 3 * pairs, off).reshape(pairs, 3)
    off += 12 * pairs
    assert off == len(buf)
    return dict(params={k: (list(v) if isinstance(v, tuple) else v) for k, v in params.items()}, result=result, pairs=pairs, optimize=calls,
                estimate=hex64(est[:8]), hessian_zeroed=int(est[8] == 0.0), null=np.packbits(null_now).tobytes().hex(),
                obs2=hex32(e21[:, :2]), info2=hex32(e21[:, 2]))


def load(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def check_against_host_build(fx, lib):
    """the fixture against rgbl_optimize_sim3_host with track_level2 = 0: return value, estimate, cleared matches, counters,
    iteration counts, bit for bit; obs2 and its information against the case.  Returns the host's result dict."""
    from orb_slam3_rgbl_amd import frontend as F
    import sim3_opt_model as sm
    case = make_case(fx["params"])
    case["track_level2"] = np.zeros(len(case["match_index"]), np.int32)
    got = F.optimize_sim3_host(case, lib)
    assert got["result"] == fx["result"] and got["n_correspondences"] == fx["pairs"], (got["result"], fx["result"], got["n_correspondences"], fx["pairs"])
    # optimize(5) with Huber on every edge, then optimize(5 or 10) without - or the return at :2349
    assert len(fx["optimize"]) == got["rounds"]
    want_calls = [[5, got["active"][0], 2 * got["active"][0], got["iterations"][0]]]
    if got["rounds"] == 2:
        want_calls.append([10 if got["n_bad"] > 0 else 5, got["active"][1], 0, got["iterations"][1]])
    assert fx["optimize"] == [[int(v) for v in c] for c in want_calls], (fx["optimize"], want_calls)
    est = np.concatenate([got["q"], got["t"], [got["s"]]])
    assert hex64(est) == fx["estimate"]
    assert fx["hessian_zeroed"] == int(got["rounds"] == 2)
    null_now = ((case["match_index"] < 0) | (got["cleared"] == 1)).astype(np.uint8)
    assert np.packbits(null_now).tobytes().hex() == fx["null"]
    # obs2 and its level, from the model's independent set-up loop: the key point of key frame 2, or the normalised point on level 0
    with np.errstate(all="ignore"):
        m = sm.Model(case)
    assert m.m == fx["pairs"] and hex32(m.obs2) == fx["obs2"] and hex32(m.info2) == fx["info2"]
    return got


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
        print("%s: result %d, pairs %d, optimize %s, %d bytes" % (name, fx["result"], fx["pairs"], fx["optimize"], os.path.getsize(path)))


if __name__ == "__main__":
    main()
