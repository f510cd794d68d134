"""rgbl_two_view_reconstruct - TwoViewReconstruction (src/TwoViewReconstruction.cc), every hypothesis of a call at once: the checks
of tests/twoview_checks.py on the CPU, with the kernel SOURCE of csrc/ransac.hip (k_tv_normalize, k_tv_hypotheses, k_tv_select,
k_tv_check_rt, k_tv_decide) running under the SIMT emulator of tests/emu against the host build of csrc/twoview_math.h, bit for bit.
tests/test_twoview_gpu.py runs the same checks on the MI355X."""
import ctypes
import os
import subprocess
import sys

import pytest

import twoview_checks as tk
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import twoview_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mt(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    yield m
    m.close()


def test_the_sets_are_drawn_from_glibc_rand():
    """GlibcRand is glibc's generator: the first values after srand(0) and after srand(12345), and RandomInt's formula"""
    libc = ctypes.CDLL("libc.so.6")
    for seed in (0, 1, 12345):
        libc.srand(seed)
        g = tc.GlibcRand(seed)
        assert [libc.rand() for _ in range(500)] == [g.rand() for _ in range(500)], seed
    sets = tc.draw_sets(100, 200)
    assert sets.shape == (200, 8) and sets.min() >= 0 and sets.max() < 100
    assert all(len(set(s)) == 8 for s in sets.tolist())
    assert sorted(tc.draw_sets(8, 1)[0].tolist()) == list(range(8))


@pytest.mark.parametrize("n_hyp", tk.NHYPS)
@pytest.mark.parametrize("N", tk.NS)
def test_every_size_against_the_host_build(emu_lib, mt, N, n_hyp):
    tk.check_size(emu_lib, mt, N, n_hyp)


def test_every_scene_and_every_exit(emu_lib, mt):
    taken = tk.check_scenes(emu_lib, mt)
    assert set(taken) == {(1, tk.FOUND), (0, tk.FOUND), (-1, tk.NO_SCORE), (0, tk.H_RATIO), (0, tk.H_RULE), (1, tk.F_FEW_OR_SIMILAR), (1, tk.F_PARALLAX)}


def test_degenerate_sets(emu_lib, mt):
    tk.check_degenerate(emu_lib, mt)


def test_ties(emu_lib, mt):
    tk.check_ties(emu_lib, mt)


def test_resident_frames_equal_host_arrays(emu_lib, mt):
    assert tk.check_forms(emu_lib, mt) > 0


@pytest.mark.parametrize("B", [1, 3, 64])
def test_batch_equals_single_calls(emu_lib, mt, B):
    assert tk.check_batch(emu_lib, mt, B) >= (1 if B == 1 else 2)


def test_error_returns_leave_the_outputs_untouched(emu_lib, mt):
    tk.check_errors(emu_lib, mt)


def test_every_size_limit_from_both_sides(emu_lib, mt):
    tk.check_limits(emu_lib, mt)


def test_most_matches(emu_lib, mt):
    assert tk.check_limit_n(emu_lib, mt) <= tk.N_MAX


def test_next_to_other_matcher_calls(emu_lib):
    tk.check_threads(emu_lib, rounds=2)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order.  It reads RGBL_EMU_ORDER once per process, so every order gets a
    process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib, frontend as F\n"
            "import twoview_checks as tk\n"
            "lib = _lib.bind(%r)\n"
            "mt = F.ORBmatcher(0.6, False, lib=lib)\n"
            "for N, h in ((65, 5), (257, 20), (300, 3)): tk.check_size(lib, mt, N, h)\n"
            "tk.check_ties(lib, mt)\n"
            "print('sizes ok')\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "sizes ok" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
