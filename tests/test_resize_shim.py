"""rgbl_shim::ImageResizer (orb_slam3_rgbl_amd/shim/ImageResizer.h) and ORBextractor::ExtractResized, compiled with the
cv_compat.h types (tests/resize_shim_test.cpp): resize() against a scalar restatement of cv::resize (a restatement, unpinned),
ScaleCalibration against the float expressions of Settings.cc:364-404 written out, the raw-image extraction against operator()
on the restated image."""
import fcntl
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "orb_slam3_rgbl_amd", "shim")
BUILD = os.path.join(ROOT, "tests", "_build")
SRCS = [os.path.join(ROOT, "tests", "resize_shim_test.cpp"), os.path.join(SHIM, "ORBextractor.cc")]


def build(libdir, libname, exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = SRCS + [os.path.join(ROOT, "include", "rgbl_frontend.h"), os.path.join(libdir, "lib%s.so" % libname)] + glob.glob(os.path.join(SHIM, "*.h"))
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            return
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-DRGBL_FORCE_CV_COMPAT", "-I" + SHIM] + SRCS +
                              ["-o", tmp, "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-pthread"])
        os.replace(tmp, exe)


def run(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "RESIZE_SHIM_OK" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


def test_cpp_resizer_under_emulation(emu_lib):
    exe = os.path.join(BUILD, "resize_shim_test_emu")
    build(BUILD, "rgbl_frontend_emu", exe)
    run(exe)


@pytest.mark.gpu
def test_cpp_resizer_on_mi355x(gpu_lib):
    exe = os.path.join(BUILD, "resize_shim_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    run(exe)
