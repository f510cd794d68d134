"""csrc/logf_glibc.h, the restatement of glibc's logf that MapPoint::PredictScale's device form evaluates, against the live
libm: bit for bit over every float of [2^-12, 2^12] (every ratio mfMaxDistance / dist the trackers can meet lies there),
over every 2^10-th positive float outside, and on the special values; and its table against the bytes of libm's own."""
import ctypes as C
import fcntl
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc", "logf_glibc.h")
BUILD = os.path.join(ROOT, "tests", "_build")


def libm():
    m = C.CDLL("libm.so.6")
    m.logf.restype, m.logf.argtypes = C.c_float, [C.c_float]
    return m


def libm_path():
    libm()
    for line in open("/proc/self/maps"):
        if "/libm.so" in line or "/libm-" in line:
            return line.split()[-1]
    raise AssertionError("libm is not mapped")


def sweep_exe():
    exe, src = os.path.join(BUILD, "logf_sweep"), os.path.join(ROOT, "tests", "logf_sweep.cpp")
    os.makedirs(BUILD, exist_ok=True)
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not (os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in (src, HEADER))):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off", "-fno-builtin", src, "-o", exe + ".tmp", "-lm"])
            os.replace(exe + ".tmp", exe)
    return exe


def test_table_constants_are_libm_bytes():
    """__logf_data = {tab[16] = {invc, logc}, ln2, poly[3]}: the header's 36 constants, in that order, are one run of bytes of libm."""
    consts = re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+", open(HEADER).read())[:36]
    blob = struct.pack("<36d", *[float.fromhex(c) for c in consts])
    assert float.fromhex(consts[18]) == 1.0 and float.fromhex(consts[19]) == 0.0      # tab[9] = {1, 0}
    assert open(libm_path(), "rb").read().count(blob) == 1


def test_every_float_of_the_working_range():
    res = subprocess.run([sweep_exe(), "dense"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "checked 201326593 mismatches 0" in res.stdout, res.stdout[-3000:]


def test_every_1024th_float_outside():
    res = subprocess.run([sweep_exe(), "sparse"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and " mismatches 0" in res.stdout and int(res.stdout.split()[1]) > 1800000, res.stdout[-3000:]


SPECIAL = np.array([0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000,
                    0xffc00000, 0x7f800001, 0xbf800000, 0x80000001, 0x3f800000, 0x3f7fffff, 0x3f800001, 0x3f330000, 0x3f32ffff,
                    0x3f99999a, 0x3f555555, 0x00400000, 0x00000100], np.uint32).view(np.float32)


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_special_values_through_the_library_hook(emu_lib):
    """zero -> -inf, negative -> NaN, inf, NaN, subnormals; NaN results are compared as NaN."""
    emu_lib.rgbl_test_logf.restype, emu_lib.rgbl_test_logf.argtypes = C.c_float, [C.c_float]
    m = libm()
    with np.errstate(all="ignore"):
        xs = np.concatenate([SPECIAL, (np.float32(1.2) ** np.arange(-9, 10)).astype(np.float32)])
    got = np.array([emu_lib.rgbl_test_logf(float(x)) for x in xs], np.float32)
    want = np.array([m.logf(float(x)) for x in xs], np.float32)
    assert same(got, want).all(), xs[~same(got, want)]
    assert got[0] == -np.inf and np.isnan(got[11]) and got[6] == np.inf and np.isnan(got[8]) and np.isfinite(got[2])
