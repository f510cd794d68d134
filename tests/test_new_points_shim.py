"""The C++ drop-in rgbl_shim::CreateNewMapPoints (orb_slam3_rgbl_amd/shim/NewMapPoints.h), compiled with stand-in KeyFrame types
(tests/new_points_shim_test.cpp): the program holds the drop-in, with host arrays and with resident frames, to a host
transcription of LocalMapping.cc:434-711 on those types; this side holds the transcription's records to the restatement with the
oracle's search, given the F12 and epipoles the drop-in computed."""
import fcntl
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import new_points_checks as nc
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "new_points_shim_test.cpp")


def build(libdir, libname, exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "tests", "shim_standins.h"), os.path.join(ROOT, "include", "rgbl_frontend.h"),
            os.path.join(libdir, "lib%s.so" % libname)] + glob.glob(os.path.join(SHIM, "*.h"))
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            return
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DRGBL_FORCE_CV_COMPAT", "-I" + SHIM,
                               SRC, "-o", tmp, "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread"])
        os.replace(tmp, exe)


def write_kf(f, kf):
    n = len(kf["desc"])
    f.write(struct.pack("<i", n))
    for key, dt in (("desc", np.uint8), ("xy", np.float32), ("octave", np.int32), ("angle", np.float32), ("uright", np.float32),
                    ("has_mp", np.uint8)):
        f.write(np.ascontiguousarray(kf[key], dt).tobytes())
    f.write(struct.pack("<i", len(kf["node_id"])))
    for key in ("node_id", "node_off", "node_feat"):
        f.write(np.ascontiguousarray(kf[key], np.int32).tobytes())
    f.write(np.ascontiguousarray(kf["scale_factors"], np.float32).tobytes())
    f.write(np.ascontiguousarray(kf["level_sigma2"], np.float32).tobytes())
    T = np.asarray(kf["Tcw"], np.float32).reshape(3, 4)
    f.write(np.ascontiguousarray(T[:, :3]).tobytes() + np.ascontiguousarray(T[:, 3]).tobytes())
    f.write(np.ascontiguousarray(T[:, :3].T).tobytes() + np.asarray(kf["Ow"], np.float32).tobytes())
    f.write(np.ascontiguousarray(kf["depth"], np.float32).tobytes() + np.ascontiguousarray(kf["xy_raw"], np.float32).tobytes())


def run_and_check(exe, lib, tmp_path):
    mt = F.ORBmatcher(0.6, False, lib=lib)
    case, _ = nc.main_fixture(mt)
    kf1, nbs, prm = case["kf1"], case["neighbours"], case["prm"]
    path, out = os.path.join(str(tmp_path), "case.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", len(nbs), prm["far_points"]))
        f.write(np.concatenate([kf1["K"], [kf1["mb"], kf1["mbf"], prm["th_far_points"], 0]]).astype(np.float32).tobytes())
        f.write(np.ascontiguousarray(case["skip"], np.uint8).tobytes())
        write_kf(f, kf1)
        for nb in nbs:
            write_kf(f, nb["kf"])
    res = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "NEW_POINTS_SHIM_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
    buf = open(out, "rb").read()
    nn = len(nbs)
    n = struct.unpack_from("<i", buf)[0]
    per = np.frombuffer(buf, np.int32, nn, 4)
    geo = np.frombuffer(buf, np.float32, 11 * nn, 4 + 4 * nn).reshape(nn, 11)
    recs = np.frombuffer(buf, L.NEW_POINT_DTYPE, n, 4 + 4 * nn + 44 * nn)
    # the restatement with the geometry the drop-in computed (F12 through rgbl_fundamental, the epipole through the stand-in camera)
    nbs2 = [dict(nb, F12=geo[i, :9], ep=geo[i, 9:]) for i, nb in enumerate(nbs)]
    want, want_per, _ = mt.CreateNewMapPointsRestatement(nc.oracle_search, kf1, nbs2, dict(prm, report_rejected=0), case["skip"])
    mt.close()
    assert n > 100
    nc.same_records(recs, want, "the transcription on the stand-in classes")
    assert np.array_equal(per, want_per)


def test_cpp_create_new_map_points_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(BUILD, "new_points_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    run_and_check(exe, emu_lib, tmp_path)


@pytest.mark.gpu
def test_cpp_create_new_map_points_on_mi355x(gpu_lib, tmp_path):
    exe = os.path.join(BUILD, "new_points_shim_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    run_and_check(exe, gpu_lib, tmp_path)
