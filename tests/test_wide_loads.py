"""The wide source windows of k_gauss7 (one 16-byte request per row and 8 columns) and k_resize_linear (one 12-byte window per
source row and 8 output columns), bit for bit against the CPU oracle: ORBextractor.image_pyramid(level, frame) against
oracle_py.Extractor.level_image, image_pyramid(level, frame, blurred=True) against level_blurred.

What the two kernels decide by a level's size, and the sizes that reach it:

  k_gauss7         a tile is 128 columns x 32 rows; a group of 8 columns is "interior" when x >= 4 and x + 12 <= W, the groups at
                   the left / right border of the level go byte by byte through the reflection (one or two groups on the right,
                   in the last tile column or - W mod 128 in 1 .. 3 - one tile earlier), the first and last tile row reflect their
                   rows.  Level widths 121 .. 141: every residue mod 8 on both sides of a tile column; 67 .. 80: the same in a
                   level of one tile.  Heights 67, 72, 96, 97, 99: a last tile row of 3 and of 8 rows, a level of whole tiles, a
                   last tile row of 1 and of 3 rows behind them.
  k_resize_linear  a pair of groups takes its 12-byte window when a start serves both groups inside the row (scale 1.1, 1.2: every
                   pair but the one the pulled-back window cannot serve at the row's end; 1.5: some pairs; 2.0: none - every
                   work-item runs its two groups on their own 8-byte windows resp. byte by byte).  Two-level extractors at these
                   scales over consecutive level-0 widths, so that the output width takes every residue mod 8 (a last pair of
                   one group, partial groups).

The extractor takes no level below 67 x 67 (one 35-px detection cell between the borders) and no cell above 72 px, so the widths 35 .. 48
and the heights 35, 40, 64, 65 of a one-tile level are shifted to the nearest sizes it accepts with the same position inside a
tile: widths 67 .. 80, heights 67, 72, 96, 97 (+ 32, the tile height; 35 and 67 fall together, 99 = 67 + 32 takes the free place).
A two-level extractor needs a level 1 of 67 px: its one-tile widths are the 16 from the smallest level 0 that gives one (74 at the
scale 1.1, 80 at 1.2, 100 at 1.5, 134 at 2.0), its heights are raised by the same amount, and at the scale 2.0 the two-tile widths
are 262 .. 277 (level 1 spans the tile column as well).

Images are uniform noise (corners on every level, so the reference blurs every level), 100 features, 2 - 3 frames per batched call
with pitch == width and single frames with pitch = width + 3 (read with the caller's odd pitch) and width + 200 (re-pitched copy).
The same checks run on the CPU emulation of the kernel sources and, marked gpu, on the device.

test_window_bounds_under_address_sanitizer: tests/wide_loads_bounds.cpp, a stand-alone program, compiled together with the kernel
sources and the SIMT emulator with -fsanitize=address (runtime linked statically), runs batches with pitch == width from exactly-sized heap blocks through
rgbl_extract_batch_device: a window that leaves the last row of the last frame is a heap-buffer-overflow there.  A plain program,
CPU only."""
import fcntl
import glob
import os
import subprocess

import numpy as np
import pytest

import parity_checks as pc
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")

WIDE = list(range(121, 142))          # both sides of the tile column at 128
NARROW = list(range(67, 81))          # a level of one tile
HEIGHTS = [67, 72, 96, 97, 99]
SCALES = [1.1, 1.2, 1.5, 2.0]
CHUNKS = 5                            # widths per parametrised case: handle creation dominates


def _noise(frames, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (frames, h, w), dtype=np.uint8)


def _compare_frame(ex, orc, img, frame, nlevels, what, kps=None, desc=None):
    okps, odesc, _ = orc(img)
    if kps is not None:
        pc.assert_keypoints_equal(kps, okps, what)
        assert np.array_equal(desc, odesc), what
    for l in range(nlevels):
        got, want = ex.image_pyramid(l, frame=frame), orc.level_image(l)
        assert got.shape == want.shape and np.array_equal(got, want), "%s: level %d differs" % (what, l)
        assert len(orc.level_keypoints(l)), "%s: no keypoint on level %d, the reference did not blur it" % (what, l)
        got, want = ex.image_pyramid(l, frame=frame, blurred=True), orc.level_blurred(l)
        assert got.shape == want.shape and np.array_equal(got, want), "%s: blurred level %d differs" % (what, l)


def check_size(lib, w, h, scale, nlevels, frames, seed):
    """One handle: a batch with pitch == width, then single frames with pitch > width."""
    what = "%dx%d scale %.1f, %d levels" % (w, h, scale, nlevels)
    ex = F.ORBextractor(100, scale, nlevels, 20, 7, w, h, max_batch=frames, lib=lib)
    orc = O.Extractor(100, scale, nlevels, 20, 7)
    imgs = _noise(frames, h, w, seed)
    res = ex.extract_batch(imgs)
    for i, (kps, desc, _) in enumerate(res):
        _compare_frame(ex, orc, imgs[i], i, nlevels, what + ", batch frame %d" % i, kps, desc)
    for pitch in (w + 3, w + 200):
        buf = np.full((h, pitch), 255, np.uint8)
        buf[:, :w] = imgs[frames - 1][::-1]
        view = buf[:, :w]
        assert view.strides == (pitch, 1)
        kps, desc, _ = ex(view)
        _compare_frame(ex, orc, view, 0, nlevels, what + ", pitch %d" % pitch, kps, desc)
    ex.close()


def _chunk(widths, k):
    return widths[k * len(widths) // CHUNKS:(k + 1) * len(widths) // CHUNKS]


def check_one_level(lib, k):
    """k_gauss7 alone: level-0 widths on both sides of a tile column and in a one-tile level, the heights in turn."""
    for n, w in enumerate(_chunk(WIDE, k) + _chunk(NARROW, k)):
        check_size(lib, w, HEIGHTS[(n + k) % len(HEIGHTS)], 1.2, 1, 2 + n % 2, 100 * k + n)


def level1(n, scale):
    """Size of level 1 as the extractor rounds it (ORBextractor.cc:1174: cvRound(width * (1 / scale)) in float)."""
    return int(np.rint(np.float32(n) * (np.float32(1.0) / np.float32(scale))))


def smallest_level0(scale):
    return next(n for n in range(67, 200) if level1(n, scale) >= 67)


def two_level_widths(scale):
    """Level-0 widths whose level 1 is accepted: the two-tile widths (twice as wide at the scale 2.0, where level 1 is to span the
    tile column too) and 16 consecutive ones from the smallest, so that level 1 takes every residue mod 8."""
    w0 = smallest_level0(scale)
    return (WIDE if scale < 2.0 else list(range(262, 278))) + list(range(w0, w0 + 16))


def check_two_levels(lib, scale, k):
    widths = two_level_widths(scale)
    assert {level1(w, scale) % 8 for w in widths} == set(range(8))
    for n, w in enumerate(_chunk(widths, k)):
        h = HEIGHTS[(n + k) % len(HEIGHTS)] + smallest_level0(scale) - 67   # level 1 is at least 67 rows
        check_size(lib, w, h, scale, 2, 2 + n % 2, 1000 * k + n)


def check_kitti(lib):
    w, h = synth.KITTI_W, synth.KITTI_H
    ex = F.ORBextractor(100, 1.2, 8, 20, 7, w, h, max_batch=2, lib=lib)
    orc = O.Extractor(100, 1.2, 8, 20, 7)
    imgs = _noise(2, h, w, 7)
    res = ex.extract_batch(imgs)
    for i, (kps, desc, _) in enumerate(res):
        _compare_frame(ex, orc, imgs[i], i, 8, "KITTI frame %d" % i, kps, desc)
    ex.close()


# ---- CPU emulation of the kernel sources ----------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_emu_one_level(emu_lib, chunk):
    check_one_level(emu_lib, chunk)


@pytest.mark.parametrize("chunk", range(CHUNKS))
@pytest.mark.parametrize("scale", SCALES)
def test_emu_two_levels(emu_lib, scale, chunk):
    check_two_levels(emu_lib, scale, chunk)


def test_emu_kitti(emu_lib):
    check_kitti(emu_lib)


# ---- the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_gpu_one_level(gpu_lib, chunk):
    check_one_level(gpu_lib, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", range(CHUNKS))
@pytest.mark.parametrize("scale", SCALES)
def test_gpu_two_levels(gpu_lib, scale, chunk):
    check_two_levels(gpu_lib, scale, chunk)


@pytest.mark.gpu
def test_gpu_kitti(gpu_lib):
    check_kitti(gpu_lib)


# ---- window bounds under AddressSanitizer (a stand-alone program, CPU only) ------------------------------------------
KERNEL_SOURCES = tuple(sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc", "*.hip"))))   # csrc/Makefile's SRCS


ASAN_FLAGS = ["-O1", "-g", "-std=c++17", "-pthread", "-ffp-contract=off", "-DRGBL_EMU", "-fsanitize=address", "-fno-sanitize-recover=all",
              "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "tests", "emu"), "-I" + os.path.join(ROOT, "include"), "-Wno-unknown-pragmas"]


def build_asan_objects():
    """Every kernel source of the library and the emulator, each compiled with -fsanitize=address: the objects the stand-alone
    programs of the suite (this file's, tests/test_alloc_fill.py's) link.  Built once, rebuilt when a source or header is newer."""
    csrc = os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc")
    emu = os.path.join(ROOT, "tests", "emu")
    srcs = [os.path.join(csrc, f) for f in KERNEL_SOURCES] + [os.path.join(emu, f) for f in ("hip_emu.cpp", "nccl_emu.cpp")]
    deps = srcs + glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(emu, "*.h")) + [os.path.join(ROOT, "include", "rgbl_frontend.h")]
    os.makedirs(BUILD, exist_ok=True)
    objs = [os.path.join(BUILD, "emu_asan.%s.o" % os.path.basename(s)) for s in srcs]
    with open(os.path.join(BUILD, "emu_asan.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        newest = max(os.path.getmtime(d) for d in deps)
        if not all(os.path.exists(o) and os.path.getmtime(o) >= newest for o in objs):
            jobs = [subprocess.Popen(["g++"] + ASAN_FLAGS + ["-c", "-x", "c++", s, "-o", o + ".tmp"], cwd=csrc) for s, o in zip(srcs, objs)]
            assert all(j.wait() == 0 for j in jobs)
            for o in objs:
                os.replace(o + ".tmp", o)
    return objs


def build_bounds_exe(program="wide_loads_bounds"):
    """tests/<program>.cpp, the kernel sources (the extractor's entry points reach into the others) and the emulator, each
    compiled with -fsanitize=address, linked into one executable with the sanitizer's runtime linked statically."""
    exe = os.path.join(BUILD, program + "_asan")
    src = os.path.join(ROOT, "tests", program + ".cpp")
    objs = build_asan_objects()
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(d) for d in objs + [src]):
            return exe
        # the sanitizer's runtime inside the executable: it starts whatever the environment preloads, and the environment stays as it is
        subprocess.check_call(["g++"] + ASAN_FLAGS + ["-static-libasan", "-x", "c++", src, "-x", "none"] + objs + ["-o", exe + ".tmp", "-ldl"])
        os.replace(exe + ".tmp", exe)
    return exe


def test_window_bounds_under_address_sanitizer():
    exe = build_bounds_exe()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and "AddressSanitizer" not in res.stderr, res.stdout[-2000:] + res.stderr[-6000:]
    assert "bounds ok" in res.stdout
