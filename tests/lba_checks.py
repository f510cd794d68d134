"""Checks of rgbl_local_bundle_adjustment shared by tests/test_lba_emu.py (the kernel SOURCE of csrc/lba.hip under the SIMT
emulator) and tests/test_lba_gpu.py (the product library on the MI355X): every output byte of the device equals
rgbl_local_bundle_adjustment_host, the host build of csrc/lba_math.h.  Each directed case first asserts, on the host build's
output, that it reached what it aims at."""
import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import lba_cases as lc

FILL = 0xAB
SCALARS = [k for k, _ in L.LbaDiag._fields_[:11]]
ARRAYS = ("cam_q", "cam_t", "point", "chi2", "flags", "q", "t", "X")


def same(a, b, what=""):
    for k in SCALARS:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.view(np.uint8).reshape(-1) != y.view(np.uint8).reshape(-1))
            raise AssertionError("%s: %s differs in %d bytes, first at byte %d" % (what, k, len(bad), bad[0]))


def untouched(r):
    """every output array still holds the fill byte"""
    return all((np.ascontiguousarray(r[k]).view(np.uint8) == FILL).all() for k in ARRAYS)


def both(lib, mt, case, what=""):
    """the host build and the device on one case; returns the host build's result after the comparison"""
    h = F.local_bundle_adjustment_host(case, lib=lib, fill=FILL)
    d = mt.LocalBundleAdjustment(case, fill=FILL)
    same(h, d, what)
    return h


# ---- the directed cases: name -> (case, what the host build's output must show) ------------------------------------------
def minimal():
    return lc.make_lba_case(n_free=1, n_fixed=1, n_points=3, obs_per_point=2, stereo_share=1.0, seed=11)


def mixed():
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=(2, 5), seed=12, outlier_share=0.12)
    c["world_pos"] = c["world_pos"].copy()
    c["world_pos"][7] = [0.3, -0.2, -25.0]   # behind every camera, and far from where its observations pull it
    return c


def single_observations():
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=30, obs_per_point=3, seed=13)
    keep = np.ones(len(c["edge_point"]), bool)
    for p, stereo in ((4, False), (9, True)):
        k = np.flatnonzero(c["edge_point"] == p)
        keep[k[1:]] = False
        c["edge_obs"] = c["edge_obs"].copy()
        if not stereo:
            c["edge_obs"][k[0], 2] = -1.0
        elif c["edge_obs"][k[0], 2] < 0:
            c["edge_obs"][k[0], 2] = c["edge_obs"][k[0], 0] - 20.0
    return lc.drop_edges(c, keep)


def initial_kf_is_the_only_fixed():
    c = lc.make_lba_case(n_free=4, n_fixed=0, n_points=40, obs_per_point=3, seed=14)
    c["free_is_fixed"] = np.array([0, 1, 0, 0], np.uint8)
    return c


def no_fixed_camera():
    return lc.make_lba_case(n_free=3, n_fixed=0, n_points=20, obs_per_point=2, seed=15)


def free_camera_without_edges():
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=3, seed=16)
    return lc.drop_edges(c, c["edge_cam"] != 1)


def point_without_edges():
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=3, seed=17)
    return lc.drop_edges(c, (c["edge_point"] != 5) & (c["edge_point"] != 39))


def points_seen_by_fixed_cameras_only():
    c = lc.make_lba_case(n_free=2, n_fixed=3, n_points=40, obs_per_point=4, seed=18)
    return lc.drop_edges(c, (c["edge_point"] >= 10) | (c["edge_cam"] >= 2))


def no_edges_at_all():
    c = lc.make_lba_case(n_free=2, n_fixed=1, n_points=5, obs_per_point=2, seed=19)
    return lc.drop_edges(c, np.zeros(len(c["edge_point"]), bool))


def tile_crossings():
    """9 free + 4 fixed cameras, 700 points, about 3 000 edges: more than 256 edges overall and on one camera, a point with 12"""
    c = lc.make_lba_case(n_free=9, n_fixed=4, n_points=700, obs_per_point=(2, 7), seed=3, outlier_share=0.03)
    first = lc.make_lba_case(n_free=9, n_fixed=4, n_points=700, obs_per_point=12, seed=3)
    k0, k1 = first["edge_point"] == 0, c["edge_point"] != 0
    for k in ("edge_point", "edge_cam", "edge_obs", "edge_inv_sigma2", "planted_outlier"):
        c[k] = np.concatenate([first[k][k0], c[k][k1]])
    c["world_pos"] = c["world_pos"].copy()
    c["world_pos"][0] = first["world_pos"][0]
    return c


def lane_sizes(n):
    """one free and one fixed camera that both see every one of n points: n edges on the camera's 64 lanes, n points on the
    per-point work-items, 2 n edges and 6 + 3 n unknowns on the 256 lanes of the whole-system sums"""
    return lc.make_lba_case(n_free=1, n_fixed=1, n_points=n, obs_per_point=2, seed=100 + n)


LANE_SIZES = (63, 64, 65, 127, 128, 129, 255, 256, 257)


def odd_totals(n_edges):
    """the 256 lanes of the whole-system sums at 255 and 257 edges (lane_sizes gives even totals only): one fixed-camera edge
    dropped from 128 / 129 points.  The unknowns, 6 per camera and 3 per point, reach 255 and 258, never 256 or 257."""
    c = lane_sizes((n_edges + 1) // 2)
    keep = np.ones(len(c["edge_point"]), bool)
    keep[np.flatnonzero(c["edge_cam"] == 1)[5]] = False
    return lc.drop_edges(c, keep)


def unknowns_255():
    return lc.make_lba_case(n_free=2, n_fixed=1, n_points=81, obs_per_point=3, seed=181)


def factor_path(n_free):
    """n_free = 20: n = 120, the last reduced system whose triangle stays in LDS; 21: the first in global memory"""
    return lc.make_lba_case(n_free=n_free, n_fixed=2, n_points=120, obs_per_point=(3, 6), seed=40 + n_free)


def far_start():
    """far off and with a lambda that lets the first steps overshoot: six rejected trials before the first accepted one and
    one more two iterations later, every one of them far from the noise floor (tests/test_lba_model.py)"""
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=(3, 5), seed=23, pose_noise=(0.1, 1.5), point_noise=4.0,
                         max_iterations=6)
    return dict(c, user_lambda_init=1e-9)


def ends_on_rejected():
    """converges, then ten trials in a row are rejected: Levenberg terminates and the edges keep the chi2 of the last of them"""
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=(3, 5), seed=21, pose_noise=(0.06, 0.8), point_noise=0.8)
    return dict(c, user_lambda_init=1e-9)


def robust_sum(case, chi2):
    stereo = ~(case["edge_obs"][:, 2] < 0)
    d = np.where(stereo, np.float32(np.sqrt(7.815)), np.float32(np.sqrt(5.991))).astype(np.float64)
    return float(np.where(chi2 <= d * d, chi2, 2 * np.sqrt(chi2) * d - d * d).sum())


def nan_observation():
    c = lc.make_lba_case(n_free=3, n_fixed=2, n_points=40, obs_per_point=3, seed=22)
    c["edge_obs"] = c["edge_obs"].copy()
    c["edge_obs"][17, 0] = np.nan
    return c


def check_directed(lib, mt, name):
    if name == "minimal":
        h = both(lib, mt, minimal(), name)
        assert h["ran"] == 1 and h["active_cams"] == 1 and h["active_points"] == 3 and h["iterations"] > 0 and h["last_chi2"] < h["first_chi2"]
    elif name == "mixed":
        c = mixed()
        h = both(lib, mt, c, name)
        stereo = ~(c["edge_obs"][:, 2] < 0)
        assert stereo.any() and (~stereo).any()
        assert (h["flags"] & 2).any(), "no edge with a depth that is not positive"
        by_chi2 = h["chi2"] > np.where(stereo, 7.815, 5.991)
        assert by_chi2.any() and ((h["flags"] & 1) == (by_chi2 | ((h["flags"] & 2) != 0))).all()
        # beyond Huber's delta: the robust sum is smaller than the plain one
        assert h["last_chi2"] < h["chi2"].sum() and h["iterations"] > 1
    elif name == "single_observations":
        c = single_observations()
        n4, n9 = (c["edge_point"] == 4).sum(), (c["edge_point"] == 9).sum()
        assert n4 == 1 and n9 == 1 and c["edge_obs"][c["edge_point"] == 4][0, 2] < 0 and c["edge_obs"][c["edge_point"] == 9][0, 2] >= 0
        h = both(lib, mt, c, name)
        assert h["failed"] == 0 and np.isfinite(h["X"]).all() and h["iterations"] > 1   # only lambda makes point 4's Hll invertible
    elif name == "initial_kf":
        c = initial_kf_is_the_only_fixed()
        h = both(lib, mt, c, name)
        assert h["ran"] == 1 and h["active_cams"] == 3 and h["iterations"] > 0
        assert h["cam_q"][1].tobytes() == both(lib, mt, dict(c, max_iterations=0))["cam_q"][1].tobytes()   # the fixed one does not move
    elif name == "no_fixed":
        h = both(lib, mt, no_fixed_camera(), name)
        assert h["ran"] == 0 and h["polls"] == 0 and untouched(h)
    elif name == "free_camera_without_edges":
        c = free_camera_without_edges()
        h = both(lib, mt, c, name)
        assert h["active_cams"] == 2 and h["iterations"] > 0
        from orb_slam3_rgbl_amd.lba_cases import f32
        q = c["cam_q"][1].astype(np.float64)
        q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        assert (h["cam_q"][1] == q.astype(f32)).all() and (h["cam_t"][1] == c["cam_t"][1]).all()   # float -> double -> float
    elif name == "point_without_edges":
        c = point_without_edges()
        h = both(lib, mt, c, name)
        assert h["active_points"] == 38 and (h["point"][5] == c["world_pos"][5]).all() and (h["point"][39] == c["world_pos"][39]).all()
        assert (h["point"][6] != c["world_pos"][6]).any()
    elif name == "fixed_only_points":
        c = points_seen_by_fixed_cameras_only()
        h = both(lib, mt, c, name)
        only_fixed = [p for p in range(10) if (c["edge_point"] == p).any()]
        assert only_fixed and h["active_points"] == len(np.unique(c["edge_point"])) and (h["point"][only_fixed] != c["world_pos"][only_fixed]).any()
    elif name == "no_edges":
        h = both(lib, mt, no_edges_at_all(), name)
        assert h["ran"] == 1 and h["iterations"] == 0 and h["polls"] == 1 and h["active_cams"] == 0 and h["active_points"] == 0
    elif name == "tile_crossings":
        c = tile_crossings()
        per_cam = np.bincount(c["edge_cam"][c["edge_cam"] < 9], minlength=9)
        assert len(c["edge_point"]) > 2800 and per_cam.max() > 256 and (c["edge_point"] == 0).sum() == 12
        h = both(lib, mt, c, name)
        assert h["active_cams"] == 9 and h["iterations"] > 1 and (h["flags"] & 1).any()
    elif name in ("edges_255", "edges_257"):
        c = odd_totals(int(name.split("_")[1]))
        assert len(c["edge_point"]) == int(name.split("_")[1])
        h = both(lib, mt, c, name)
        assert h["iterations"] > 1 and h["active_cams"] == 1
    elif name == "unknowns_255":
        h = both(lib, mt, unknowns_255(), name)
        assert 6 * h["active_cams"] + 3 * h["active_points"] == 255 and h["iterations"] > 1
    elif name in ("factor_42", "factor_43"):   # n = 252 / 258: around the 256 rows one pass of k_lba_factor's work-items covers
        n_free = int(name.split("_")[1])
        h = both(lib, mt, dict(lc.make_lba_case(n_free=n_free, n_fixed=2, n_points=150, obs_per_point=(4, 8), seed=n_free), max_iterations=2), name)
        assert h["active_cams"] == n_free and h["failed"] == 0 and h["iterations"] == 2
    elif name.startswith("factor_"):
        n_free = int(name.split("_")[1])
        h = both(lib, mt, factor_path(n_free), name)
        assert h["active_cams"] == n_free and h["failed"] == 0 and h["iterations"] > 1 and h["last_chi2"] < h["first_chi2"]
    elif name == "rejected_trials":
        h = both(lib, mt, far_start(), name)
        assert h["rejected"] > 0 and h["trials"] > h["iterations"] > 1
    elif name == "ends_on_rejected":
        c = ends_on_rejected()
        h = both(lib, mt, c, name)
        assert h["iterations"] < 10 and h["rejected"] >= 10 and h["failed"] == 0
        assert abs(robust_sum(c, h["chi2"]) - h["last_chi2"]) > 1e-9 * h["last_chi2"]   # the flags read the rejected step's chi2
        ok = both(lib, mt, dict(c, user_lambda_init=0.0))
        assert abs(robust_sum(c, ok["chi2"]) - ok["last_chi2"]) <= 1e-9 * ok["last_chi2"]
    elif name == "nan_observation":
        h = both(lib, mt, nan_observation(), name)
        # every factorisation fails; every iteration ends on its one rejected trial, whose chi2 the flags read
        assert h["failed"] == h["trials"] == h["rejected"] == h["iterations"] == 10 and np.isnan(h["chi2"][17]) and np.isnan(h["last_chi2"])
        assert not (h["flags"][17] & 1) and h["point"].tobytes() == nan_observation()["world_pos"].tobytes()
    elif name == "user_lambda_init":
        c = mixed()
        h0, h = both(lib, mt, c), both(lib, mt, dict(c, user_lambda_init=100.0), name)
        assert h["X"].tobytes() != h0["X"].tobytes()
        one, one0 = both(lib, mt, dict(c, user_lambda_init=100.0, max_iterations=1)), both(lib, mt, dict(c, max_iterations=1))
        assert one["rejected"] == 0 and 33.3 < one["last_lambda"] < 66.7 and one["last_lambda"] != one0["last_lambda"]   # 100 x [1/3, 2/3]
    elif name == "max_iterations":
        c = mixed()
        h = both(lib, mt, dict(c, max_iterations=0), name)
        assert h["ran"] == 1 and h["iterations"] == 0 and h["polls"] == 1 and (h["chi2"] == 0).all() and (h["flags"][c["edge_point"] == 7] == 3).all()
        assert (h["point"] == c["world_pos"]).all()
        h = both(lib, mt, dict(c, max_iterations=1), name)
        assert h["iterations"] == 1 and h["polls"] >= 2 and (h["chi2"] > 0).any()
    else:
        raise KeyError(name)


DIRECTED = ("minimal", "mixed", "single_observations", "initial_kf", "no_fixed", "free_camera_without_edges", "point_without_edges",
            "fixed_only_points", "no_edges", "tile_crossings", "factor_20", "factor_21", "factor_42", "factor_43", "edges_255", "edges_257", "unknowns_255", "rejected_trials", "ends_on_rejected", "nan_observation",
            "user_lambda_init", "max_iterations")


def check_lane_size(lib, mt, n):
    h = both(lib, mt, lane_sizes(n), "lane size %d" % n)
    assert h["active_cams"] == 1 and h["active_points"] == n and h["iterations"] > 1


def check_stop(lib, mt):
    """the flag set at entry; then every poll of a run with rejected trials as the poll at which the flag becomes set - the
    iteration starts and the polls inside the trial loop alike"""
    c = far_start()
    h = both(lib, mt, dict(c, stop=np.array([1], np.int32)), "stop set at entry")
    assert h["ran"] == 0 and h["polls"] == 1 and untouched(h)
    h = both(lib, mt, dict(c, stop_byte=np.array([1], np.uint8)), "stop_byte set at entry")   # the flag as a C++ bool
    assert h["ran"] == 0 and h["polls"] == 1 and untouched(h)
    assert both(lib, mt, dict(c, stop_byte=np.array([0], np.uint8), stop=np.array([0], np.int32)))["ran"] == 1
    full = both(lib, mt, dict(c, stop=np.array([0], np.int32)), "stop not set")
    assert full["polls"] > full["iterations"] + 1, "no poll inside a trial loop"
    at_start = in_trials = 0
    prev = None
    for n in range(1, full["polls"] + 1):
        h = both(lib, mt, dict(c, stop_after_polls=n), "stop_after_polls %d" % n)
        # a stop inside a trial loop is read once more by the iteration loop's condition (sparse_optimizer.cpp:376)
        assert h["polls"] in (n, n + 1) and h["ran"] == (1 if n > 1 else 0) and h["iterations"] <= full["iterations"]
        if prev is not None and prev["ran"]:
            at_start += h["iterations"] == prev["iterations"] + 1 and h["rejected"] == prev["rejected"]   # one more whole iteration ran
            in_trials += h["rejected"] == prev["rejected"] + 1 and h["iterations"] - prev["iterations"] in (0, 1)   # it ended on a rejected trial
        prev = h
    assert at_start > 0 and in_trials > 0
    return full["polls"]


def check_pool(lib, mt):
    c = mixed()
    n = len(c["world_pos"])
    rng = np.random.default_rng(5)
    slot = rng.permutation(3 * n)[:n].astype(np.int32)
    pool = F.MapPointPool(3 * n, lib=lib)
    try:
        others = np.setdiff1d(np.arange(3 * n), slot).astype(np.int32)
        marks = rng.normal(size=(len(others), 3)).astype(np.float32)
        pool.update(others, world_pos=marks)

        def load():
            pool.update(slot, world_pos=c["world_pos"])
        pc = {k: v for k, v in c.items() if k != "world_pos"}
        pc.update(pool=pool, slot=slot, n_points=n)
        load()
        h = F.local_bundle_adjustment_host(c, lib=lib, fill=FILL)
        d = mt.LocalBundleAdjustment(pc, fill=FILL)
        same(h, d, "pool form")
        assert pool.download(slot)["world_pos"].tobytes() == h["point"].tobytes()      # what Refresh(.., true, false) reads
        assert pool.download(others)["world_pos"].tobytes() == marks.tobytes()
        # untouched after ran = 0, after the stop at :1406 and after an error
        for what, change in (("no fixed camera", dict(n_fixed=0, n_free=5, free_is_fixed=None)), ("stop", dict(stop_after_polls=1)),
                             ("error", dict(edge_cam=np.where(np.arange(len(c["edge_cam"])) == 3, 99, c["edge_cam"]).astype(np.int32)))):
            load()
            call = mt.prepare_LocalBundleAdjustment(dict(pc, **change), fill=FILL)
            try:
                r = call()
                assert what != "error" and r["ran"] == 0
            except L.RgblError as e:
                assert what == "error" and e.code == L.ERR_INVALID
            assert untouched(call.outputs), what
            assert pool.download(slot)["world_pos"].tobytes() == c["world_pos"].tobytes(), what
        # a slot outside the pool, a slot listed twice
        for bad in (np.where(np.arange(n) == 2, 3 * n, slot), np.where(np.arange(n) == 2, slot[0], slot)):
            call = mt.prepare_LocalBundleAdjustment(dict(pc, slot=bad.astype(np.int32)), fill=FILL)
            try:
                call()
                raise AssertionError("a bad slot was accepted")
            except L.RgblError as e:
                assert e.code == L.ERR_INVALID
            assert untouched(call.outputs)
    finally:
        pool.close()


def refused(lib, mt, case, host=True, device=True):
    """RGBL_ERR_INVALID from both builds, every output untouched"""
    calls = []
    if host:
        calls.append(F.local_bundle_adjustment_call(lib, None, case, FILL))
    if device:
        calls.append(mt.prepare_LocalBundleAdjustment(case, FILL))
    for call in calls:
        try:
            call()
        except L.RgblError as e:
            assert e.code == L.ERR_INVALID, e
        else:
            raise AssertionError("accepted")
        assert untouched(call.outputs)
        raw = bytes(memoryview(call.raw))
        assert all(b == FILL for b in raw[5 * 8:5 * 8 + 8 * 4 + 3 * 8]), "the diag's scalars were written"


def check_errors(lib, mt):
    c = mixed()
    nE, nC, nP = len(c["edge_point"]), 5, 40
    def at(a, i, v):
        a = np.array(a, copy=True)
        a.reshape(-1)[i] = v
        return a
    refused(lib, mt, dict(c, edge_point=at(c["edge_point"], nE - 1, nP)))
    refused(lib, mt, dict(c, edge_point=at(c["edge_point"], 0, -1)))
    refused(lib, mt, dict(c, edge_cam=at(c["edge_cam"], 5, nC)))
    refused(lib, mt, dict(c, edge_cam=at(c["edge_cam"], 5, -1)))
    k = int(np.flatnonzero(np.diff(c["edge_point"]) > 0)[3]) + 1      # the first edge of a point
    refused(lib, mt, dict(c, edge_point=at(c["edge_point"], k, c["edge_point"][k] - 2)))      # decreasing
    same_pt = int(np.flatnonzero(np.diff(c["edge_point"]) == 0)[0])
    refused(lib, mt, dict(c, edge_cam=at(c["edge_cam"], same_pt + 1, c["edge_cam"][same_pt])))   # a repeated (point, camera) pair
    for key, i in (("cam_q", 6), ("cam_t", 13), ("cam_K", 2), ("cam_bf", 4)):
        for v in (np.nan, np.inf):
            refused(lib, mt, dict(c, **{key: at(c[key], i, v)}))
    zq = np.array(c["cam_q"], copy=True)
    zq[4] = 0.0
    refused(lib, mt, dict(c, cam_q=zq))   # an all-zero quaternion has no rotation
    for key in ("cam_q", "cam_t", "cam_K", "cam_bf", "world_pos", "edge_point", "edge_cam", "edge_obs", "edge_inv_sigma2"):
        refused(lib, mt, dict(c, **{key: None}, n_points=nP, n_edges=nE))
    for key in ("n_free", "n_fixed", "n_points", "n_edges"):
        refused(lib, mt, dict(c, **{key: -1}))
    pool = F.MapPointPool(64, lib=lib)
    try:
        refused(lib, mt, dict({k: v for k, v in c.items() if k != "world_pos"}, pool=pool, slot=np.arange(nP, dtype=np.int32), n_points=nP),
                device=False)   # the host build reads host arrays only
    finally:
        pool.close()


def check_limits(lib, mt, device_inside=True):
    """every limit from both sides: the highest count runs (max_iterations = 1), one more is refused"""
    # n_free
    c = lc.make_lba_case(n_free=128, n_fixed=2, n_points=300, obs_per_point=(3, 6), seed=60, max_iterations=1)
    h = both(lib, mt, c, "n_free = 128")
    assert h["active_cams"] == 128 and h["iterations"] == 1 and h["failed"] == 0
    c = lc.make_lba_case(n_free=129, n_fixed=2, n_points=30, obs_per_point=3, seed=61)
    refused(lib, mt, c)
    # n_fixed
    small = lc.make_lba_case(n_free=2, n_fixed=2, n_points=20, obs_per_point=3, seed=62, max_iterations=1)
    def with_fixed(n):
        reps = n - 2
        return dict(small, n_fixed=n, cam_q=np.concatenate([small["cam_q"], np.tile(small["cam_q"][3], (reps, 1))]),
                    cam_t=np.concatenate([small["cam_t"], np.tile(small["cam_t"][3], (reps, 1))]),
                    cam_K=np.concatenate([small["cam_K"], np.tile(small["cam_K"][3], (reps, 1))]),
                    cam_bf=np.concatenate([small["cam_bf"], np.tile(small["cam_bf"][3], reps)]))
    c = with_fixed(1024)
    c["edge_cam"] = np.where(c["edge_cam"] == 3, 2 + 1023, c["edge_cam"]).astype(np.int32)    # the highest camera index in use
    assert (c["edge_cam"] == 1025).any()
    h = both(lib, mt, c, "n_fixed = 1024")
    assert h["iterations"] == 1
    refused(lib, mt, with_fixed(1025))
    # n_points and n_edges: 2^18 points with four observations each are 2^20 edges
    nP, per = 1 << 18, 4
    base = lc.make_lba_case(n_free=2, n_fixed=2, n_points=64, obs_per_point=4, seed=63, max_iterations=1)
    assert len(base["edge_point"]) == 64 * per
    reps = nP // 64
    big = dict(base, world_pos=np.tile(base["world_pos"], (reps, 1)),
               edge_point=(np.tile(base["edge_point"], reps) + np.repeat(np.arange(reps, dtype=np.int32) * 64, 64 * per)).astype(np.int32),
               edge_cam=np.tile(base["edge_cam"], reps), edge_obs=np.tile(base["edge_obs"], (reps, 1)),
               edge_inv_sigma2=np.tile(base["edge_inv_sigma2"], reps))
    assert len(big["edge_point"]) == 1 << 20 and big["edge_point"][-1] == nP - 1
    h = both(lib, mt, big, "2^18 points, 2^20 edges") if device_inside else F.local_bundle_adjustment_host(big, lib=lib, fill=FILL)
    assert h["iterations"] == 1 and h["active_points"] == nP and np.isfinite(h["point"]).all()
    more_pts = dict(big, world_pos=np.concatenate([big["world_pos"], big["world_pos"][:1]]))
    refused(lib, mt, more_pts)
    more_edges = dict(big, edge_point=np.append(big["edge_point"], nP - 1).astype(np.int32), edge_cam=np.append(big["edge_cam"], 0).astype(np.int32),
                      edge_obs=np.concatenate([big["edge_obs"], big["edge_obs"][:1]]), edge_inv_sigma2=np.append(big["edge_inv_sigma2"], 1).astype(np.float32))
    more_edges["edge_cam"][-1] = 3 if big["edge_cam"][-1] != 3 else 2
    refused(lib, mt, more_edges)
