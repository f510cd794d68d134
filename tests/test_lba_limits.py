"""The size limits of rgbl_local_bundle_adjustment from both sides under the emulator: n_free = 128 and n_fixed = 1024 run on
the emulated kernels, 2^18 points with 2^20 edges on the host build (tests/test_lba_gpu.py runs them on the MI355X), and one
more of each is refused by both builds with every output untouched."""
import pytest

import lba_checks as lk
from orb_slam3_rgbl_amd import frontend as F


def test_every_limit_from_both_sides(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    try:
        lk.check_limits(emu_lib, m, device_inside=False)
    finally:
        m.close()
