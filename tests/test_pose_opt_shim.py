"""The C++ drop-in rgbl_shim::PoseOptimization (orb_slam3_rgbl_amd/shim/PoseOptimizer.h), compiled with stand-in Frame / MapPoint
types (tests/pose_opt_shim_test.cpp): the program runs it with host arrays and with a resident frame + DeviceLocalMap (equal
results), below three correspondences, and on a rig frame and a fisheye camera (refused); this side holds the pose, flags and
return value it left to the C ABI's host build (bit for bit), to the planted pose, and to the planted outliers."""
import fcntl
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_opt_model as pm
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "pose_opt_shim_test.cpp")


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


def run_and_check(exe, lib, tmp_path):
    case = cases.make_pose_opt_case(500, 300, seed=3)
    n = len(case["mp_index"])
    pos = np.zeros((n, 3), np.float32)
    has = case["mp_index"] >= 0
    pos[has] = case["world_pos"][case["mp_index"][has]]
    path, out = os.path.join(str(tmp_path), "case.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", n, int(case["n_levels"])))
        for a, dt in ((case["mp_index"], np.int32), (pos, np.float32), (case["xy"], np.float32), (case["octave"], np.int32),
                      (case["uright"], np.float32), (case["q"], np.float32), (case["t"], np.float32), (case["K"], np.float32),
                      (case["bf"], np.float32), (case["inv_level_sigma2"], np.float32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "POSE_OPT_SHIM_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    buf = open(out, "rb").read()
    result = struct.unpack_from("<i", buf)[0]
    q, t = np.frombuffer(buf, np.float32, 4, 4), np.frombuffer(buf, np.float32, 3, 20)
    flags = np.frombuffer(buf, np.uint8, n, 32)
    # the drop-in is the C ABI: the host build's bits
    want = F.pose_optimization_host(case, lib, outlier_fill=1)
    assert result == want["result"] and np.array_equal(flags, want["outlier"])
    assert np.array_equal(q.view(np.uint32), want["q"].view(np.uint32)) and np.array_equal(t.view(np.uint32), want["t"].view(np.uint32))
    # the planted pose: the entry pose is 0.15 m and 0.01 rad away; what comes back is at least three times closer on both counts
    Rt, R = pm.quat_to_rot(case["q_true"]), pm.quat_to_rot(q)
    angle = np.arccos(np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1))
    dist = np.linalg.norm(t.astype(np.float64) - case["t_true"])
    print("recovered pose: %.2e rad, %.2e m from the planted one" % (angle, dist))
    assert angle < 0.01 / 3 and dist < 0.15 / 3
    # the planted outliers: at most the model's own disagreement with the plant
    model = pm.run(case)
    mine = int((flags[has] != case["planted_outlier"][has]).sum())
    assert mine <= int((model["outlier"][has] != case["planted_outlier"][has]).sum())
    assert (flags[~has] == 1).all()   # stale flags of features without a map point stay


def test_cpp_pose_optimization_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(BUILD, "pose_opt_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    run_and_check(exe, emu_lib, tmp_path)


@pytest.mark.gpu
def test_cpp_pose_optimization_on_mi355x(gpu_lib, tmp_path):
    exe = os.path.join(BUILD, "pose_opt_shim_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    run_and_check(exe, gpu_lib, tmp_path)
