"""RGBL_GBA_PANEL: the panel width of rgbl_bundle_adjustment's solve is read once, when the matcher is created, and the result's
bits do not depend on it.  Each width of the switch (16, 64; 32 is what every other test runs) gets a fresh process that runs
directed cases of tests/gba_checks.py - device == host build in every output byte - on sizes that cross one, two and three
panels of that width, a failed pivot in a later panel, and one case past LocalBundleAdjustment's cap."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("panel_2", "panel_3", "panel_5", "panel_6", "panel_10", "panel_11", "panel_17", "panel_21", "panel_22", "panel_33", "one_camera",
         "failed_pivot_in_a_later_panel", "nan_observation", "past_lba_cap")
SCRIPT = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import gba_checks as gk
from orb_slam3_rgbl_amd import _lib, frontend as F
lib = _lib.bind(sys.argv[1]) if sys.argv[1] != "product" else _lib.load()
mt = F.ORBmatcher(0.6, False, lib=lib)
for name in sys.argv[2:]:
    gk.check_directed(lib, mt, name)
mt.close()
print("GBA_WIDTH_OK", len(sys.argv) - 2)
"""


def run_width(width, lib_path):
    env = dict(os.environ, RGBL_GBA_PANEL=str(width))
    res = subprocess.run([sys.executable, "-c", SCRIPT % (ROOT, os.path.join(ROOT, "tests")), lib_path] + list(CASES), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and "GBA_WIDTH_OK %d" % len(CASES) in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]


@pytest.mark.parametrize("width", [16, 64])
def test_every_width_of_the_switch_gives_the_host_builds_bits(emu_lib, width):
    run_width(width, os.path.join(ROOT, "tests", "_build", "librgbl_frontend_emu.so"))


@pytest.mark.gpu
@pytest.mark.parametrize("width", [16, 64])
def test_every_width_of_the_switch_gives_the_host_builds_bits_on_mi355x(gpu_lib, width):
    run_width(width, "product")
