"""Writes tests/golden/pose_opt/host_bits.json and tests/golden/sim3_opt/host_bits.json: what rgbl_pose_optimization_host and
rgbl_optimize_sim3_host of the emulator library (the host build of csrc/poseopt_math.h and csrc/sim3opt_math.h on the CPU)
return on the cases of tests/host_bits.py.  Run it BEFORE a change that must keep the bits, never after: the records are the
yardstick of tests/test_host_bits.py and of the recorded-bits tests on the MI355X.
Run from the repository root:  python tests/golden/make_host_bits.py"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import host_bits as hb  # noqa: E402
from orb_slam3_rgbl_amd import _lib  # noqa: E402
from orb_slam3_rgbl_amd import frontend as F  # noqa: E402


def main():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc"), "emu"])
    lib = _lib.bind(os.path.join(ROOT, "tests", "_build", "librgbl_frontend_emu.so"))
    pose = {name: hb.pose_record(F.pose_optimization_host(case, lib, outlier_fill=hb.FILL)) for name, case, _ in hb.pose_cases()}
    sim3 = {name: hb.sim3_record(F.optimize_sim3_host(case, lib, cleared_fill=hb.FILL)) for name, case, _ in hb.sim3_cases()}
    for which, rec in (("pose_opt", pose), ("sim3_opt", sim3)):
        json.dump(rec, open(hb.path(which), "w"), indent=1, sort_keys=True)
        print("%s: %d cases" % (hb.path(which), len(rec)))


if __name__ == "__main__":
    main()
