"""The host-fed batch front end driven from C++ through the C ABI alone (tests/feed_test.cpp: rgbl_feeder_* in the frame loop of
Examples/RGB-L/rgbl_kitti.cc, raw BGR and .bin bytes read from files straight into the page-locked slots), every frame held to
the single-frame ABI calls.  CPU: against the SIMT-emulation library; `-m gpu`: the product library at KITTI size."""
import fcntl
import os
import subprocess

import pytest

import feed_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "feed_test.cpp")


def build(libdir, libname, exe):
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [SRC, os.path.join(ROOT, "include", "rgbl_frontend.h"), os.path.join(libdir, "lib%s.so" % libname)]
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in deps):
            return
        tmp = "%s.tmp.%d" % (exe, os.getpid())
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-o", tmp,
                               "-L" + libdir, "-l" + libname, "-Wl,-rpath," + libdir])
        os.replace(tmp, exe)


def write_frames(d, lib, w, h, lengths, seed):
    with open(os.path.join(d, "proj.txt"), "w") as f:
        f.write(" ".join(repr(float(v)) for v in fc.projection(lib, w, h).reshape(-1)))
    imgs = fc.colour_frames(seed, w, h, len(lengths), 3)
    for i, n in enumerate(lengths):
        imgs[i].tofile(os.path.join(d, "frame_%06d.bgr" % i))
        fc.bin_scan(seed + i, n).tofile(os.path.join(d, "scan_%06d.bin" % i))


def run(exe, d, w, h, nfeatures, nlevels, frames, batch, slots, max_points):
    res = subprocess.run([exe, str(d), str(w), str(h), str(nfeatures), str(nlevels), str(frames), str(batch), str(slots),
                          str(max_points)], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("FEED_CPP_OK")][-1].split()
    return int(line[1]), int(line[2]), int(line[3])


def test_feed_from_cpp_under_emulation(emu_lib, tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "feed_test_emu")
    build(os.path.join(ROOT, "tests", "_build"), "rgbl_frontend_emu", exe)
    lengths = [1200, 0, 700, 1500, 1, 900, 1023]
    write_frames(str(tmp_path), emu_lib, 320, 200, lengths, seed=4)
    frames, kps, hits = run(exe, tmp_path, 320, 200, 300, 4, len(lengths), 2, 2, 1500)
    assert frames == len(lengths) and kps > 300 and hits > 5


@pytest.mark.gpu
def test_feed_from_cpp_on_the_gpu(gpu_lib, tmp_path):
    exe = os.path.join(ROOT, "tests", "_build", "feed_test_gpu")
    build(os.path.join(ROOT, "orb_slam3_rgbl_amd"), "rgbl_frontend", exe)
    lengths = [130000, 0, 121000, 115000, 1, 129000, 90000, 125000, 118000, 127000, 122000, 1025, 116000, 128000, 119000, 130000,
               124000, 117000, 0, 126000]
    write_frames(str(tmp_path), gpu_lib, 1241, 376, lengths, seed=9)
    frames, kps, hits = run(exe, tmp_path, 1241, 376, 2000, 8, len(lengths), 8, 3, 130000)
    assert frames == len(lengths) and kps > 1000 * len(lengths) and hits > 1000
