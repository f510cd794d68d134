"""The C++ drop-in ORBmatcher::SearchLocalPoints and rgbl_shim::DeviceLocalMap (orb_slam3_rgbl_amd/shim/ORBmatcher.h,
LocalMap.h), compiled with stand-in Frame / MapPoint types (tests/local_map_shim_test.cpp): the program holds the drop-in,
with and without the device-resident local map, to a literal host transcription of Tracking.cc:3399-3448 on those types;
this side holds the transcription's results to the restatement and the oracle."""
import fcntl
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import local_map_checks as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "local_map_shim_test.cpp")
TH = 3.0


def build(libdir, libname, exe, extra=()):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "rgbl_frontend.h"), os.path.join(libdir, "lib%s.so" % libname)] + glob.glob(os.path.join(SHIM, "*.h"))
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            return
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DRGBL_FORCE_CV_COMPAT"] + list(extra) +
                              [SRC, "-o", tmp, "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread"])
        os.replace(tmp, exe)


def the_case(n1=None):
    """the shared case as the C++ program lists it: entry 33 of the local map is point 5 once more"""
    case, _ = lc.base_case()
    n1 = n1 or len(case["world_pos1"])
    idx = np.arange(n1)
    if n1 > 40:
        idx[33] = 5
    return lc.take_points(case, idx), idx


def write_case(path, case):
    n1, n2 = len(case["world_pos1"]), len(case["kp2_xy"])
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", n1, n2, len(case["scale_factors"]), int(case["far_points"])))
        fl = np.concatenate([[TH, case["th_far_points"]], case["grid"], case["Rcw"], case["tcw"], case["Ow"], case["K"],
                             [case["mbf"], case["log_scale_factor"]]]).astype(np.float32)
        fl = np.concatenate([fl, np.zeros(30 - len(fl), np.float32)])
        f.write(fl.tobytes())
        f.write(np.ascontiguousarray(case["scale_factors"], np.float32).tobytes())
        for key, dt in (("world_pos1", np.float32), ("normal1", np.float32), ("min_dist1", np.float32), ("max_dist1", np.float32),
                        ("mp_desc1", np.uint8), ("mp_observed1", np.uint8), ("consider1", np.uint8), ("kp2_xy", np.float32),
                        ("kp2_octave", np.int32), ("uright2", np.float32), ("desc2", np.uint8), ("blocked2", np.uint8)):
            f.write(np.ascontiguousarray(case[key], dt).tobytes())


def run_and_check(exe, tmp_path):
    case, idx = the_case()
    path, out = os.path.join(str(tmp_path), "case.bin"), os.path.join(str(tmp_path), "out.bin")
    write_case(path, case)
    res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "LOCAL_MAP_SHIM_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    # the transcription's results against restatement + oracle
    buf = open(out, "rb").read()
    n1, n2, n_to_match, ret = struct.unpack_from("<4i", buf)
    pos = 16

    def take(dt, n):
        nonlocal pos
        a = np.frombuffer(buf, dt, n, pos)
        pos += a.nbytes
        return a
    in_view, level, visible = take(np.int32, n1), take(np.int32, n1), take(np.int32, n1)
    px, py, pxr, depth, vcos = [take(np.float32, n1) for _ in range(5)]
    match = take(np.int32, n2)
    wiv, wrec, wn, wm, wnm = lc.expected_fused(case, TH, 0.8)
    cons = case["consider1"] != 0
    assert n1 == len(wiv) and n_to_match == wn and ret == wnm and wnm > 60
    assert np.array_equal(in_view[cons] != 0, wiv[cons] != 0)
    assert lc.same(px[cons], wrec["proj_x"][cons]) and lc.same(py[cons], wrec["proj_y"][cons])
    seen = wiv != 0
    for got, fld in ((pxr, "proj_xr"), (depth, "depth"), (vcos, "view_cos")):
        assert lc.same(got[seen], wrec[fld][seen]), fld
    assert np.array_equal(level[seen], wrec["level"][seen])
    # fields of points that were not considered, and the last four of a point that is not in view, keep their stale values
    assert (px[~cons] == -7).all() and np.array_equal(in_view[~cons], (idx % 2)[~cons]) and (level[cons & ~seen] == -7).all() and (depth[cons & ~seen] == -7).all()
    want_visible = 1 + np.array([int(wiv[idx == idx[i]].sum()) for i in range(n1)])
    assert np.array_equal(visible, want_visible)
    assert np.array_equal(match, np.where(wm == 33, 5, wm))


def test_cpp_search_local_points_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(BUILD, "local_map_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    run_and_check(exe, tmp_path)


def test_cpp_local_map_threads_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(BUILD, "local_map_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    case, _ = the_case(400)
    path = os.path.join(str(tmp_path), "case.bin")
    write_case(path, case)
    for mode in ("threads", "abi_threads"):
        res = subprocess.run([exe, path, os.path.join(str(tmp_path), "out.bin"), mode], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "LOCAL_MAP_SHIM_OK" in res.stdout, mode + res.stdout[-3000:] + res.stderr[-3000:]


@pytest.mark.skipif(not os.environ.get("RGBL_TSAN"), reason="minutes under ThreadSanitizer: RGBL_TSAN=1 runs it, as for tests/test_shim_threads.py")
def test_cpp_local_map_threads_under_thread_sanitizer(oracle, tmp_path):
    """TSan clean: a search on slots [0, n) next to updates, erases and growth on other slots of the same pool - through the
    drop-in classes, and on the C ABI itself (the scenario of local_map_checks.check_threads, which a Python process cannot run
    under the sanitizer)."""
    import test_shim_threads
    test_shim_threads.build_tsan_emulator()
    exe = os.path.join(BUILD, "local_map_shim_test_tsan")
    build(BUILD, "rgbl_frontend_emu_thread", exe, extra=("-fsanitize=thread",))
    case, _ = the_case(120)
    path = os.path.join(str(tmp_path), "case.bin")
    write_case(path, case)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66 second_deadlock_stack=1")
    for mode in ("threads", "abi_threads"):   # a process each: the emulator's fibers count against the sanitizer's thread limit
        res = subprocess.run([exe, path, os.path.join(str(tmp_path), "out.bin"), mode], capture_output=True, text=True, timeout=1500, env=env)
        assert res.returncode == 0 and "LOCAL_MAP_SHIM_OK" in res.stdout, mode + res.stdout[-3000:] + res.stderr[-6000:]
        assert "ThreadSanitizer" not in res.stderr, mode + res.stderr[-6000:]


@pytest.mark.gpu
def test_cpp_search_local_points_on_mi355x(gpu_lib, tmp_path):
    exe = os.path.join(BUILD, "local_map_shim_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    run_and_check(exe, tmp_path)
