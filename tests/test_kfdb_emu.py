"""KeyFrameDatabase: the checks of tests/kfdb_checks.py on the CPU, with the kernel SOURCES of csrc/kfdb.hip running under the
SIMT emulator of tests/emu.  This checks kernel and host logic against the restatement of the reference (tests/kfdb_ref.py),
not the MI355X; tests/test_kfdb_gpu.py runs the same checks there."""
import os
import subprocess
import sys

import pytest

import kfdb_checks as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_against_restatement_1_to_2000_entries(emu_lib):
    kc.check_query_sizes(emu_lib)


def test_empty_database_and_disjoint_query(emu_lib):
    kc.check_empty_and_disjoint(emu_lib)


def test_ties_strict_threshold_and_floor(emu_lib):
    kc.check_ties_and_threshold(emu_lib)


def test_excluded_sets(emu_lib):
    kc.check_excluded(emu_lib)


def test_erase_readd_clear_map_order(emu_lib):
    kc.check_mutation_order(emu_lib)


def test_compaction_changes_no_result(emu_lib):
    kc.check_compaction(emu_lib)


def test_arena_growth(emu_lib):
    kc.check_arena_growth(emu_lib)


def test_batch_equals_single_queries(emu_lib):
    kc.check_batch(emu_lib)


def test_error_returns(emu_lib):
    kc.check_errors(emu_lib)


def test_detect_mirrors_end_to_end(emu_lib):
    kc.check_detect(emu_lib)


def test_vocabulary_to_candidates(emu_lib):
    kc.check_vocabulary_end_to_end(emu_lib)


def test_threaded_add_erase_query(emu_lib):
    kc.check_threads(emu_lib)


@pytest.mark.parametrize("order", ["asc", "desc", "shuffle"])
def test_kernels_are_schedule_independent(emu_lib, order):
    """The emulator resumes work-items in another order: a missing barrier in the staging or the term hand-off shows here.
    The emulator reads RGBL_EMU_ORDER once per process, so every order gets a process of its own."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from orb_slam3_rgbl_amd import _lib\n"
            "import kfdb_checks as kc\n"
            "lib = _lib.bind(%r)\n"
            "print('scored', kc.check_query_sizes(lib, sizes=(70, 300), places=(1, 2)))\n"
            "kc.check_batch(lib)\n" % (ROOT, os.path.join(ROOT, "tests"), emu_lib._name))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RGBL_EMU_ORDER=order), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "scored" in res.stdout, res.stdout[-1500:] + res.stderr[-3000:]
