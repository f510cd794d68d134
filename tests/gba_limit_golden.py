"""Writes tests/golden/gba/limit_1024.npz: the case of tests/test_gba_limits.py at the cap of 1 024 active cameras (one
iteration, 600 points) together with what tests/lba_model.py, extended by tests/gba_model.py, makes of it - the plain
run's R, t and X and the model's own reordering noise (edges permuted, and solved with the Schur complement, against the plain
run; tests/golden/lba/README.md).  The model assembles the full normal equations densely (10 644 unknowns) and takes most of a
minute for its three runs, so the GPU test reads this record instead of running it.

    python tests/gba_limit_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from orb_slam3_rgbl_amd import lba_cases as lc  # noqa: E402

INPUTS = ("cam_is_fixed", "cam_q", "cam_t", "cam_K", "cam_bf", "world_pos", "edge_point", "edge_cam", "edge_obs", "edge_inv_sigma2")
PATH = os.path.join(HERE, "golden", "gba", "limit_1024.npz")


def limit_case():
    c = lc.make_ba_case(n_cams=1025, n_fixed=1, n_points=600, obs_per_point=14, seed=70, step=0.01, max_iterations=1)
    assert len(np.unique(c["edge_cam"])) == 1025, "a camera without an edge"
    return c


def main():
    import gba_model as T
    case = limit_case()
    base, perm, schur = T.three_runs(case)
    assert base["iterations"] == 1 and base["accepted"] == [True] and base["failed"] == 0
    rec = {k: np.asarray(case[k]) for k in INPUTS}
    for key in ("R", "t", "X"):
        b = base[key]
        floor = 2.0 ** -52 * max(float(np.abs(b).max()), 1.0)
        rec[key] = b
        rec["noise_" + key] = np.float64(max(float(np.abs(perm[key] - b).max()), float(np.abs(schur[key] - b).max()), floor))
        print(key, "noise", rec["noise_" + key])
    rec["first_chi2"], rec["last_chi2"] = np.float64(base["first_chi2"]), np.float64(base["last_chi2"])
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **rec)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
