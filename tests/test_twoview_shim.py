"""The C++ drop-in rgbl_shim::TwoViewReconstruction (shim/TwoViewReconstruction.h) on stand-in cv / Eigen / Sophus types
(tests/twoview_shim_glue.cpp), run on the scenes of the fixtures under tests/golden/two_view - the recorded runs of the reference's
own compiled functions (tests/twoview_golden.py).  Needs nothing of the reference: the inputs are regenerated from the fixtures'
parameters.  One object per fixture runs its calls one after the other.  Checked per call: the sets the drop-in draws are the sets
the reference's DUtils::Random drew (its own glibc generator, seeded as SeedRandOnce(0), the stream going on from call to call);
the return value, T21 and vbTriangulated are the recorded bits; vP3D is assigned exactly where the reference assigns it - not on
the homography path - and holds the recorded bits; with the constructor flag it is assigned on the homography path too, with the
winning hypothesis's points; scores, n_good and parallax are the recorded ones.  With the emulated kernels here, and on the MI355X."""
import os
import subprocess

import numpy as np
import pytest

import twoview_golden as tg
from sim3_golden import hexf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
BUILD = os.path.join(TESTS, "_build")


def build_shim(lib_path, tag):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "twoview_shim_" + tag)
    glue = os.path.join(TESTS, "twoview_shim_glue.cpp")
    deps = [glue, os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim", "TwoViewReconstruction.h"), os.path.join(ROOT, "include", "rgbl_frontend.h"), lib_path]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = exe + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", tmp, "-I" + os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim"),
                               "-I" + os.path.join(ROOT, "include"), glue, lib_path, "-Wl,-rpath," + os.path.dirname(lib_path)])
        os.replace(tmp, exe)
    return exe


def run(exe, fx, assign):
    params = fx["params"]
    its = params["iterations"]
    cs, blob = tg.run(exe, params, ok="TWOVIEW_SHIM_OK", extra_args=["1" if assign else "0"])
    n1 = len(cs[0]["xy1"])
    at, paths = 0, []
    for k, call in enumerate(fx["calls"]):
        head = np.frombuffer(blob, np.int32, 8, at); at += 32
        S = np.frombuffer(blob, np.float32, 2, at); at += 8
        T = np.frombuffer(blob, np.float32, 12, at); at += 48
        n_good = np.frombuffer(blob, np.int32, 8, at); at += 32
        par = np.frombuffer(blob, np.float32, 8, at); at += 32
        sets = np.frombuffer(blob, np.int32, its * 8, at); at += its * 32
        flags = np.frombuffer(blob, np.uint8, n1, at); at += n1
        p3d = np.frombuffer(blob, np.float32, int(head[7]) * 3, at); at += int(head[7]) * 12
        what = "call %d" % k
        assert [int(v) for v in sets] == call["sets"], (what, "the sets are not the ones the reference drew")
        assert int(head[0]) == call["ret"] and hexf(S[:1]) == call["SH"] and hexf(S[1:]) == call["SF"], what
        model = int(head[1])
        if call["ret"]:
            assert hexf(T) == call["T21"] and flags.tobytes().hex() == call["tri"], what
        else:
            assert (flags == 7).all() and head[7] == 0, what
        if model == 1:
            assert [int(v) for v in n_good[:4]] == call["f_n_good"] and hexf(par[:4]) == call["f_parallax"], what
        if call["ret"] and model == 1:
            assert head[7] == n1 == call["p3d_size"] and hexf(p3d) == call["p3d"], what
        elif call["ret"] and assign:       # the homography path with the flag: the winner's points, at the triangulated keys at least
            assert head[7] == n1 and call["p3d_size"] == 0 and np.abs(p3d.reshape(-1, 3)[flags == 1]).max() > 0, what
        else:
            assert head[7] == 0 == call["p3d_size"], (what, "vP3D was assigned")
        paths.append((model, call["ret"]))
    assert at == len(blob)
    return paths


def check(lib_path, tag):
    exe = build_shim(lib_path, tag)
    seen = []
    for name in sorted(tg.CASES):
        fx = tg.load(name)
        a, b = run(exe, fx, False), run(exe, fx, True)
        assert a == b and a[-1][0] == tg.CASES[name]["last"][0], (name, a)
        seen += a
    assert (1, 1) in seen and (0, 1) in seen and (1, 0) in seen and (0, 0) in seen and (-1, 0) in seen, seen
    return seen


def test_drop_in_reproduces_the_fixtures_on_the_emulator(emu_lib):
    check(emu_lib._name, "emu")


@pytest.mark.gpu
def test_drop_in_reproduces_the_fixtures_on_mi355x(gpu_lib):
    check(os.path.join(ROOT, "orb_slam3_rgbl_amd", "librgbl_frontend.so"), "gpu")
