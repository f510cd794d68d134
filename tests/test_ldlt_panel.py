"""lm_solve_panel of csrc/lm_math.h, the host text of the global bundle adjustment's solve, against lm_solve_n: the stand-alone
program tests/ldlt_panel_test.cpp (no library, no device), once plain and once under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "ldlt_panel_test.cpp")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]), ("sanitized", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_panel_solve_equals_lm_solve_n_but_for_the_backward_order(name, flags, tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(str(tmp_path), "ldlt_panel_test_" + name)
    subprocess.check_call(["g++", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-ffp-contract=off", "-I" + CSRC, SRC, "-o", exe] + flags)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "LDLT_PANEL_OK 24 cases" in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
