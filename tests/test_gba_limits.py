"""The size limits of rgbl_bundle_adjustment from both sides: the highest count runs, one more is refused by both builds with
every output untouched.

    cameras listed        2 048 run (most of them without an edge, the highest index in use) / 2 049
    cameras flagged fixed 1 024 / 1 025
    active cameras        1 024 / 1 025.  At 1 024 the reduced system has 6 144 unknowns; the host build is cubic in that and
                          would not end in seconds, so the DEVICE is held against the float64 LAPACK model instead, within
                          16 x the model's own noise as recorded in tests/golden/gba/limit_1024.npz (tests/gba_limit_golden.py
                          writes it; margin and procedure of tests/golden/lba/README.md).  GPU tier only: the emulator would
                          take minutes.
    points, edges         2^18, 2^20 / one more of each
    pairs of edges        more than 2^27 pairs that share a point are refused.  The inside of this bound is 1 GiB of lists
                          behind a reduced system of thousands of unknowns and is not run here.

The CPU tier runs the inside of the caps on the emulated kernels where the active set is small, and 2^18 points on the host
build alone; tests marked gpu run them on the MI355X."""
import numpy as np
import pytest

import gba_checks as gk
import lba_model as M
from gba_limit_golden import INPUTS, PATH, limit_case
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import lba_cases as lc

MARGIN = 16.0


def with_cameras(c, n, n_flagged):
    """c with copies of its camera 0 appended up to n cameras - none of them has an edge -, the first n_flagged of them fixed"""
    reps = n - int(c["n_cams"])
    fixed = np.concatenate([c["cam_is_fixed"], (np.arange(reps) < n_flagged).astype(np.uint8)])
    return dict(c, n_cams=n, cam_is_fixed=fixed, cam_q=np.concatenate([c["cam_q"], np.tile(c["cam_q"][0], (reps, 1))]),
                cam_t=np.concatenate([c["cam_t"], np.tile(c["cam_t"][0], (reps, 1))]),
                cam_K=np.concatenate([c["cam_K"], np.tile(c["cam_K"][0], (reps, 1))]),
                cam_bf=np.concatenate([c["cam_bf"], np.tile(c["cam_bf"][0], reps)]))


def check_camera_counts(lib, mt):
    small = lc.make_ba_case(n_cams=4, n_fixed=2, n_points=20, obs_per_point=3, seed=62, max_iterations=1)
    c = with_cameras(small, 2048, 1022)   # 2 + 1022 = 1 024 fixed
    assert c["cam_is_fixed"].sum() == 1024
    # the highest camera index in use: a fixed camera's edges go to a fixed copy of camera 0 ... whose pose is camera 0's
    c["edge_cam"] = np.where(c["edge_cam"] == 0, 4 + 1021, c["edge_cam"]).astype(np.int32)
    key = np.lexsort((c["edge_cam"], c["edge_point"]))
    for k in ("edge_point", "edge_cam", "edge_obs", "edge_inv_sigma2"):
        c[k] = c[k][key]
    assert (c["edge_cam"] == 1025).any() and c["cam_is_fixed"][1025] == 1
    last = dict(c, edge_cam=np.where(c["edge_cam"] == 1025, 2047, c["edge_cam"]).astype(np.int32))   # ... and to the last one listed (free)
    for case, active in ((c, 2), (last, 3)):
        h = gk.both(lib, mt, case, "n_cams = 2048")
        assert h["iterations"] == 1 and h["active_cams"] == active
    gk.refused(lib, mt, with_cameras(small, 2049, 1022))
    gk.refused(lib, mt, with_cameras(small, 2048, 1023))   # 1 025 fixed


def one_past_the_active_cap():
    c = lc.make_ba_case(n_cams=1026, n_fixed=1, n_points=600, obs_per_point=14, seed=70, step=0.01, max_iterations=1)
    assert len(np.unique(c["edge_cam"])) == 1026
    return c


def check_points_and_edges(lib, mt, device_inside):
    nP, per = 1 << 18, 4
    base = lc.make_ba_case(n_cams=4, n_fixed=2, n_points=64, obs_per_point=4, seed=63, max_iterations=1)
    assert len(base["edge_point"]) == 64 * per
    reps = nP // 64
    big = dict(base, world_pos=np.tile(base["world_pos"], (reps, 1)),
               edge_point=(np.tile(base["edge_point"], reps) + np.repeat(np.arange(reps, dtype=np.int32) * 64, 64 * per)).astype(np.int32),
               edge_cam=np.tile(base["edge_cam"], reps), edge_obs=np.tile(base["edge_obs"], (reps, 1)),
               edge_inv_sigma2=np.tile(base["edge_inv_sigma2"], reps))
    assert len(big["edge_point"]) == 1 << 20 and big["edge_point"][-1] == nP - 1
    h = gk.both(lib, mt, big, "2^18 points, 2^20 edges") if device_inside else F.bundle_adjustment_host(big, lib=lib, fill=gk.FILL)
    assert h["iterations"] == 1 and h["active_points"] == nP and np.isfinite(h["point"]).all() and (h["included"] == 1).all()
    gk.refused(lib, mt, dict(big, world_pos=np.concatenate([big["world_pos"], big["world_pos"][:1]])))
    more = dict(big, edge_point=np.append(big["edge_point"], nP - 1).astype(np.int32), edge_cam=np.append(big["edge_cam"], 0).astype(np.int32),
                edge_obs=np.concatenate([big["edge_obs"], big["edge_obs"][:1]]), edge_inv_sigma2=np.append(big["edge_inv_sigma2"], 1).astype(np.float32))
    gk.refused(lib, mt, more)


def too_many_pairs():
    """256 points that all 1 024 free cameras (and the fixed one) observe: 256 x 1 024 x 1 025 / 2 pairs, 131 072 past 2^27"""
    one = lc.make_ba_case(n_cams=1025, n_fixed=1, n_points=1, obs_per_point=1025, seed=64, step=0.01, max_iterations=1)
    assert len(one["edge_point"]) == 1025
    n = 256
    c = dict(one, world_pos=np.tile(one["world_pos"], (n, 1)), edge_point=np.repeat(np.arange(n, dtype=np.int32), 1025),
             edge_cam=np.tile(one["edge_cam"], n), edge_obs=np.tile(one["edge_obs"], (n, 1)), edge_inv_sigma2=np.tile(one["edge_inv_sigma2"], n))
    assert n * 1024 * 1025 // 2 > 1 << 27 and len(c["edge_point"]) <= 1 << 20
    return c


def check_limits(lib, mt, device_inside):
    check_camera_counts(lib, mt)
    gk.refused(lib, mt, one_past_the_active_cap())
    gk.refused(lib, mt, too_many_pairs())
    check_points_and_edges(lib, mt, device_inside)


def test_every_limit_from_both_sides(emu_lib):
    m = F.ORBmatcher(0.6, False, lib=emu_lib)
    try:
        check_limits(emu_lib, m, device_inside=False)
    finally:
        m.close()


def test_the_recorded_case_is_the_generated_one():
    rec, case = np.load(PATH), limit_case()
    for k in INPUTS:
        assert rec[k].tobytes() == np.asarray(case[k]).tobytes(), k


@pytest.mark.gpu
def test_every_limit_from_both_sides_on_mi355x(gpu_lib):
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    try:
        check_limits(gpu_lib, m, device_inside=True)
    finally:
        m.close()


@pytest.mark.gpu
def test_1024_active_cameras_within_the_models_recorded_noise(gpu_lib):
    rec = np.load(PATH)
    case = dict({k: rec[k] for k in INPUTS}, n_cams=1025, robust=1, max_iterations=1)
    m = F.ORBmatcher(0.6, False, lib=gpu_lib)
    try:
        d = m.BundleAdjustment(case, fill=gk.FILL)
    finally:
        m.close()
    assert (d["active_cams"], d["iterations"], d["trials"], d["rejected"], d["failed"]) == (1024, 1, 1, 0, 0)
    R = np.array([M.rot_of_quat(q) for q in d["q"]]).reshape(1025, 3, 3)
    for key, got in (("R", R), ("t", d["t"]), ("X", d["X"])):
        noise, diff = float(rec["noise_" + key]), float(np.abs(got - rec[key]).max())
        print("%s: noise %.3g diff %.3g" % (key, noise, diff))
        assert diff <= MARGIN * noise, (key, diff, noise)
    assert d["last_chi2"] < d["first_chi2"]
