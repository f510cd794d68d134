"""The C++ drop-in rgbl_shim::Sim3Solver (orb_slam3_rgbl_amd/shim/Sim3Solver.h), compiled with stand-in KeyFrame / MapPoint / matrix
types (tests/sim3_shim_test.cpp).  The program checks the overloads, find, SolveBatch, a DeviceLocalMap, the early exits and the
refusal of a fisheye camera against each other.  This side compares what its calls of iterate(20, ...) left with the fixtures
under tests/golden/sim3 - what the reference's own Sim3Solver.cc and DUtils::Random did on the same case after srand(seed)
(tests/sim3_golden.py): the triples in the order drawn, mRansacMaxIts, per call bNoMore, bConverge, nInliers, mnIterations,
mnBestInliers, the matrix and vbInliers through mvnIndices1, bit for bit - and replays every call through rgbl_sim3_ransac_host
with mnBestInliers carried over.  The one documented deviation is measured too: the rand() values a converged call used beyond
the reference's."""
import fcntl
import glob
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import sim3_golden as sg
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "sim3_shim_test.cpp")


def build(libdir, libname, exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "rgbl_frontend.h"), os.path.join(libdir, "lib%s.so" % libname)] + glob.glob(os.path.join(SHIM, "*.h"))
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            return
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DRGBL_FORCE_CV_COMPAT", "-I" + SHIM,
                               SRC, "-o", tmp, "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread"])
        os.replace(tmp, exe)


def max_iterations(n, min_inliers, limit=300, prob=0.99):
    """SetRansacParameters (:134-144)"""
    if min_inliers == n:
        return 1
    eps = float(np.float32(min_inliers) / np.float32(n))
    if eps ** 3 >= 1:   # log of zero or of a negative number: the quotient is 0 or NaN, and max(1, ...) makes either one iteration
        return 1
    return max(1, min(int(math.ceil(math.log(1 - prob) / math.log(1 - eps ** 3))), limit))


def replay(name, out_path, lib):
    """the calls the program recorded against the fixture of the reference's own run, and through rgbl_sim3_ransac_host"""
    fx = sg.load(name)
    assert fx["params"] == sg.CASES[name]
    c = sg.shim_case(**fx["params"])
    buf = open(out_path, "rb").read()
    n, n1 = len(c["where"]), c["n1"]
    max_its, N, n_calls, raw_draws = struct.unpack_from("<4i", buf)
    off = 16
    assert N == n == fx["N"] and max_its == fx["max_its"] == max_iterations(n, c["min_inliers"])
    assert n_calls == len(fx["calls"])
    best, iterations, converged, total_drawn = 0, 0, False, 0
    best_T = np.eye(4, dtype=np.float32)
    for k, ref in enumerate(fx["calls"]):
        drawn, no_more, conv, inliers, its_after, best_after = struct.unpack_from("<6i", buf, off)
        off += 24
        samples = np.frombuffer(buf, np.int32, 3 * drawn, off).reshape(drawn, 3)
        off += 12 * drawn
        T = np.frombuffer(buf, np.float32, 16, off).reshape(4, 4)
        off += 64
        flags = np.frombuffer(buf, np.uint8, n1, off)
        off += n1
        total_drawn += drawn
        assert not converged, "a call after the solver converged"
        # what the reference's own code did in this call
        assert (no_more, conv, inliers, its_after, best_after) == (ref["no_more"], ref["converge"], ref["inliers"], ref["iterations"], ref["best"]), k
        assert sg.hexbits(flags) == ref["flags"], k
        if n < c["min_inliers"]:   # :225-229: over before anything is drawn
            assert drawn == 0 and sg.hexf(T) == ref["T"] == sg.IDENTITY
            continue
        # the sampling order: this call draws every triple it may use, the reference only those it used - the same ones
        assert drawn == min(sg.STEP, max_its - iterations) >= ref["ran"]
        assert [int(v) for v in samples[:ref["ran"]].reshape(-1)] == ref["triples"], "call %d: the triples are not the reference's" % k
        assert (drawn == ref["ran"]) or conv, k
        # a converged call returns the reference's matrix; any other returns mBestT12, where the reference returns bestSim3 -
        # mBestT12 if the call held a hypothesis, else never written (zero in the stand-in)
        assert sg.hexf(T) == (ref["T"] if conv else ref["best_T12"]) and ref["T"] in (ref["best_T12"], sg.ZERO), k
        # and the host build on ALL the triples drawn
        res = F.sim3_ransac_host(dict(c["pr"], samples=samples, n_hyp=drawn, best_inliers=best), lib)
        iterations += res["iterations_run"]
        if res["selected"] >= 0:
            best, best_T = res["n_inliers"], res["T12"]
        assert (its_after, best_after) == (iterations, best) and conv == res["converged"], k
        if conv:
            full = np.zeros(n1, np.uint8)
            full[c["where"]] = res["inlier"]
            assert np.array_equal(flags, full), k
        assert T.tobytes() == np.asarray(best_T, np.float32).tobytes(), k
        converged = bool(conv)
    assert off == len(buf)
    # the documented deviation: every triple drawn took three rand() values, so after a convergence before the call's last
    # iteration the stream is further along than the reference's, which drew 3 * mnIterations
    assert raw_draws == 3 * total_drawn >= 3 * iterations
    assert (raw_draws > 3 * iterations) == (converged and total_drawn > iterations)
    return n_calls, converged, raw_draws - 3 * iterations


def run_and_check(exe, lib, tmp_path):
    seen = {}
    for name in sorted(sg.CASES):
        c = sg.shim_case(**sg.CASES[name])
        path, out = os.path.join(str(tmp_path), "case_%s.bin" % name), os.path.join(str(tmp_path), "out_%s.bin" % name)
        sg.write_case(c, path)
        res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "SIM3_SHIM_OK" in res.stdout, name + ": " + res.stdout[-3000:] + res.stderr[-3000:]
        seen[name] = replay(name, out, lib)
    return seen


def test_cpp_sim3_solver_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(BUILD, "sim3_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    seen = run_and_check(exe, emu_lib, tmp_path)
    print(seen)
    assert seen["converges"][1] and seen["converges"][2] > 0 and not seen["runs_through"][1] and seen["runs_through"][2] == 0


@pytest.mark.gpu
def test_cpp_sim3_solver_on_mi355x(gpu_lib, tmp_path):
    exe = os.path.join(BUILD, "sim3_shim_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    seen = run_and_check(exe, gpu_lib, tmp_path)
    assert seen["converges"][1] and seen["converges"][2] > 0
