"""Checks of rgbl_bundle_adjustment shared by tests/test_gba_emu.py (the kernel SOURCE of csrc/gba.hip and csrc/lba.hip under the
SIMT emulator) and tests/test_gba_gpu.py (the product library on the MI355X): every output byte of the device equals
rgbl_bundle_adjustment_host, the host build of csrc/lba_math.h with lm_solve_panel.  Each directed case first asserts, on the
host build's output, that it reached what it aims at.

The sizes are the smallest at which a panel schedule can go wrong.  With W columns per panel (kLmPanel of csrc/lm_math.h, read
from the header) and n = 6 nA unknowns they are the multiples of 6 next to W - 6, W, W + 6, 2 W and 3 W + 6: one partial
panel; the last one below W and the first above; around 2 W; 3 W + 6, which has a partial last panel behind three full ones."""
import os
import re

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import lba_cases as lc

FILL = 0xAB
SCALARS = [k for k, _ in L.LbaDiag._fields_[:11]]
ARRAYS = ("cam_q", "cam_t", "point", "included", "chi2", "q", "t", "X")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = int(re.search(r"constexpr int kLmPanel = (\d+);", open(os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc", "lm_math.h")).read()).group(1))


def panel_sizes():
    """nA for n = 6 nA next to W - 6, W (below and above), W + 6, 2 W (below and above), 3 W and 3 W + 6"""
    below = lambda n: n // 6
    above = lambda n: -(-n // 6)
    return sorted({max(1, below(W - 6)), below(W), above(W), above(W + 6), below(2 * W), above(2 * W), above(3 * W), above(3 * W + 6)})


PANEL_SIZES = panel_sizes()


def same(a, b, what=""):
    for k in SCALARS:
        assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (what, k, a[k], b[k])
    for k in ARRAYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.view(np.uint8).reshape(-1) != y.view(np.uint8).reshape(-1))
            raise AssertionError("%s: %s differs in %d bytes, first at byte %d" % (what, k, len(bad), bad[0]))


def untouched(r):
    return all((np.ascontiguousarray(r[k]).view(np.uint8) == FILL).all() for k in ARRAYS)


def both(lib, mt, case, what=""):
    """the host build and the device on one case; returns the host build's result after the comparison"""
    h = F.bundle_adjustment_host(case, lib=lib, fill=FILL)
    d = mt.BundleAdjustment(case, fill=FILL)
    same(h, d, what)
    return h


def sized(nA, n_fixed=1, **kw):
    """nA free cameras that all have edges, n_fixed fixed ones"""
    kw.setdefault("n_points", 30 + 8 * nA)
    kw.setdefault("obs_per_point", (3, 6))
    kw.setdefault("seed", 200 + nA)
    kw.setdefault("max_iterations", 3)
    c = lc.make_ba_case(n_cams=nA + n_fixed, n_fixed=n_fixed, **kw)
    assert len(np.unique(c["edge_cam"])) == nA + n_fixed, "a camera without an edge"
    return c


def mixed(**kw):
    return lc.make_ba_case(n_cams=5, n_fixed=1, n_points=40, obs_per_point=(2, 5), seed=12, outlier_share=0.12, **kw)


def far_start():
    """so far off that computeLambdaInit's own lambda lets steps overshoot (the reference sets no other): four rejected trials in
    six iterations"""
    return lc.make_ba_case(n_cams=5, n_fixed=2, n_points=40, obs_per_point=(3, 5), seed=28, pose_noise=(0.2, 3.0), point_noise=6.0,
                           max_iterations=6)


def huber_sum(case, chi2, mono=5.99):
    """the robust chi2 sum with thHuber2D = sqrt(mono) (Optimizer.cc:131: 5.99; LocalBundleAdjustment has 5.991)"""
    stereo = ~(case["edge_obs"][:, 2] < 0)
    d = np.where(stereo, np.float32(np.sqrt(7.815)), np.float32(np.sqrt(mono))).astype(np.float64)
    return float(np.where(chi2 <= d * d, chi2, 2 * np.sqrt(chi2) * d - d * d).sum())


def check_directed(lib, mt, name):
    if name.startswith("panel_"):
        nA = int(name.split("_")[1])
        h = both(lib, mt, sized(nA), name)
        assert h["ran"] == 1 and h["active_cams"] == nA and h["failed"] == 0 and h["iterations"] == 3 and h["last_chi2"] < h["first_chi2"]
    elif name == "one_camera":
        h = both(lib, mt, sized(1, n_points=12, obs_per_point=2), name)
        assert h["active_cams"] == 1 and h["failed"] == 0 and h["last_chi2"] < h["first_chi2"]
    elif name == "past_lba_cap":
        c = sized(129, n_points=400, max_iterations=1)
        h = both(lib, mt, c, name)
        assert h["active_cams"] == 129 and h["failed"] == 0 and h["iterations"] == 1
        for handle in (None, mt.h):   # LocalBundleAdjustment still refuses what is one past ITS cap
            call = F.local_bundle_adjustment_call(lib, handle, lc.as_lba_case(c), FILL)
            try:
                call()
                raise AssertionError("rgbl_local_bundle_adjustment accepted 129 free cameras")
            except L.RgblError as e:
                assert e.code == L.ERR_INVALID
    elif name in ("robust", "plain"):
        c = mixed(robust=1 if name == "robust" else 0)
        h = both(lib, mt, c, name)
        assert h["iterations"] > 1 and h["failed"] == 0
        plain, huber = float(h["chi2"].sum()), huber_sum(c, h["chi2"])
        assert huber < plain * (1 - 1e-6), "no edge beyond Huber's delta: the case does not tell the two apart"
        want, other = (huber, plain) if name == "robust" else (plain, huber)
        assert abs(h["last_chi2"] - want) <= 1e-9 * want and abs(h["last_chi2"] - other) > 1e-6 * other
        if name == "robust":   # thHuber2D is sqrt(5.99) here (:131), not LocalBundleAdjustment's sqrt(5.991): the sums tell them apart
            mono = c["edge_obs"][:, 2] < 0
            assert (h["chi2"][mono] > 5.991).any()
            assert abs(h["last_chi2"] - huber_sum(c, h["chi2"], mono=5.991)) > 1e-7 * want
    elif name in ("monocular", "stereo", "mixed_edges"):
        share = dict(monocular=0.0, stereo=1.0, mixed_edges=0.5)[name]
        c = lc.make_ba_case(n_cams=6, n_fixed=1, n_points=60, obs_per_point=(3, 5), seed=31, stereo_share=share)
        if name == "stereo":   # a right coordinate left of the image reads as a monocular edge
            c = lc.drop_edges(c, ~(c["edge_obs"][:, 2] < 0))
        mono = c["edge_obs"][:, 2] < 0
        assert mono.all() if name == "monocular" else (~mono).all() if name == "stereo" else (mono.any() and (~mono).any())
        h = both(lib, mt, c, name)
        assert h["active_cams"] == 5 and h["failed"] == 0 and h["iterations"] > 1 and h["last_chi2"] < h["first_chi2"]
    elif name == "free_camera_without_edges":
        c = lc.make_ba_case(n_cams=5, n_fixed=1, n_points=40, obs_per_point=3, seed=16)
        c = lc.drop_edges(c, c["edge_cam"] != 2)
        h = both(lib, mt, c, name)
        assert h["active_cams"] == 3 and h["iterations"] > 0
        q = c["cam_q"][2].astype(np.float64)
        q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        assert (h["cam_q"][2] == q.astype(np.float32)).all() and (h["cam_t"][2] == c["cam_t"][2]).all()   # float -> double -> float
        assert (h["cam_t"][3] != c["cam_t"][3]).any()
    elif name == "point_without_edges":
        c = lc.make_ba_case(n_cams=5, n_fixed=1, n_points=40, obs_per_point=3, seed=17)
        c = lc.drop_edges(c, (c["edge_point"] != 5) & (c["edge_point"] != 39))
        h = both(lib, mt, c, name)
        want = np.ones(40, np.uint8)
        want[[5, 39]] = 0
        assert h["active_points"] == 38 and (h["included"] == want).all()
        assert (h["point"][5] == c["world_pos"][5]).all() and (h["point"][39] == c["world_pos"][39]).all() and (h["point"][6] != c["world_pos"][6]).any()
    elif name == "no_fixed_camera":
        c = sized(4, n_fixed=0, max_iterations=4)
        assert not c["cam_is_fixed"].any()
        h = both(lib, mt, c, name)   # the gauge is free: Levenberg's lambda alone makes the system definite
        assert h["ran"] == 1 and h["active_cams"] == 4 and h["iterations"] > 0 and (h["cam_t"] != c["cam_t"]).any()
    elif name == "rejected_trials":
        c = far_start()
        h = both(lib, mt, c, name)
        assert h["rejected"] > 0 and h["trials"] > h["iterations"] > 1
    elif name == "nan_observation":
        c = lc.make_ba_case(n_cams=5, n_fixed=2, n_points=40, obs_per_point=3, seed=22)
        c["edge_obs"] = c["edge_obs"].copy()
        c["edge_obs"][17, 0] = np.nan
        h = both(lib, mt, c, name)
        # every factorisation fails: tempChi = DBL_MAX, x persists (zeros), every iteration ends on its one rejected trial
        assert h["failed"] == h["trials"] == h["rejected"] == h["iterations"] == 10 and np.isnan(h["chi2"][17]) and np.isnan(h["last_chi2"])
        assert h["point"].tobytes() == c["world_pos"].tobytes()
    elif name == "failed_pivot_in_a_later_panel":
        # the NaN reaches only the LAST camera's diagonal block (its point keeps no other free observer): every panel before
        # that camera's columns factorises, the pivot fails in the last one and the substitutions must not run
        nA = PANEL_SIZES[-1]
        c = sized(nA, max_iterations=2)
        k = int(np.flatnonzero(c["edge_cam"] == nA)[0])
        c = lc.drop_edges(c, (c["edge_point"] != c["edge_point"][k]) | (c["edge_cam"] == nA) | (c["edge_cam"] == 0))
        k = int(np.flatnonzero(c["edge_cam"] == nA)[0])
        c["edge_obs"] = c["edge_obs"].copy()
        c["edge_obs"][k, 0] = np.nan
        assert 6 * (nA - 1) >= 2 * W and len(np.unique(c["edge_cam"])) == nA + 1
        h = both(lib, mt, c, name)
        assert h["active_cams"] == nA and h["failed"] == h["trials"] == 2 and h["point"].tobytes() == c["world_pos"].tobytes()
    elif name == "max_iterations":
        c = mixed()
        h = both(lib, mt, dict(c, max_iterations=0), name)
        assert h["ran"] == 1 and h["iterations"] == 0 and h["polls"] == 0 and (h["chi2"] == 0).all() and (h["point"] == c["world_pos"]).all()
        for n in (5, 20):
            h = both(lib, mt, dict(c, max_iterations=n), name)
            assert 1 <= h["iterations"] <= n
    else:
        raise KeyError(name)


DIRECTED = tuple("panel_%d" % n for n in PANEL_SIZES) + (
    "one_camera", "past_lba_cap", "robust", "plain", "monocular", "stereo", "mixed_edges", "free_camera_without_edges",
    "point_without_edges", "no_fixed_camera", "rejected_trials", "nan_observation", "failed_pivot_in_a_later_panel", "max_iterations")


def check_stop(lib, mt):
    """the flag set at entry is no early return here: optimize() runs, polls once and ends; then every poll of a run with
    rejected trials as the poll at which the flag becomes set"""
    c = far_start()
    for form in (dict(stop=np.array([1], np.int32)), dict(stop_byte=np.array([1], np.uint8))):
        h = both(lib, mt, dict(c, **form), "stop set at entry")
        assert h["ran"] == 1 and h["polls"] == 1 and h["iterations"] == 0 and not untouched(h)
        assert (h["point"] == c["world_pos"]).all() and (h["included"] == 1).all() and (h["chi2"] == 0).all()
    full = both(lib, mt, dict(c, stop=np.array([0], np.int32), stop_byte=np.array([0], np.uint8)), "stop not set")
    assert full["polls"] > full["iterations"] + 1, "no poll inside a trial loop"
    at_start = in_trials = 0
    prev = None
    for n in range(1, full["polls"] + 1):
        h = both(lib, mt, dict(c, stop_after_polls=n), "stop_after_polls %d" % n)
        assert h["polls"] in (n, n + 1) and h["ran"] == 1 and h["iterations"] <= full["iterations"]
        if prev is not None:
            at_start += h["iterations"] == prev["iterations"] + 1 and h["rejected"] == prev["rejected"]
            in_trials += h["rejected"] == prev["rejected"] + 1 and h["iterations"] - prev["iterations"] in (0, 1)
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
        pc = {k: v for k, v in c.items() if k != "world_pos"}
        pc.update(pool=pool, slot=slot, n_points=n)
        pool.update(slot, world_pos=c["world_pos"])
        h = F.bundle_adjustment_host(c, lib=lib, fill=FILL)
        d = mt.BundleAdjustment(pc, fill=FILL)
        same(h, d, "pool form")
        assert pool.download(slot)["world_pos"].tobytes() == h["point"].tobytes()
        assert pool.download(others)["world_pos"].tobytes() == marks.tobytes()
        # an error, a slot outside the pool and a slot listed twice leave the pool and the outputs untouched
        bad_cam = np.where(np.arange(len(c["edge_cam"])) == 3, 99, c["edge_cam"]).astype(np.int32)
        for change in (dict(edge_cam=bad_cam), dict(slot=np.where(np.arange(n) == 2, 3 * n, slot).astype(np.int32)),
                       dict(slot=np.where(np.arange(n) == 2, slot[0], slot).astype(np.int32))):
            pool.update(slot, world_pos=c["world_pos"])
            call = mt.prepare_BundleAdjustment(dict(pc, **change), fill=FILL)
            try:
                call()
                raise AssertionError("accepted")
            except L.RgblError as e:
                assert e.code == L.ERR_INVALID
            assert untouched(call.outputs)
            assert pool.download(slot)["world_pos"].tobytes() == c["world_pos"].tobytes()
    finally:
        pool.close()


def refused(lib, mt, case, host=True, device=True):
    """RGBL_ERR_INVALID from both builds, every output untouched"""
    calls = []
    if host:
        calls.append(F.bundle_adjustment_call(lib, None, case, FILL))
    if device:
        calls.append(mt.prepare_BundleAdjustment(case, FILL))
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
    k = int(np.flatnonzero(np.diff(c["edge_point"]) > 0)[3]) + 1
    refused(lib, mt, dict(c, edge_point=at(c["edge_point"], k, c["edge_point"][k] - 2)))
    same_pt = int(np.flatnonzero(np.diff(c["edge_point"]) == 0)[0])
    refused(lib, mt, dict(c, edge_cam=at(c["edge_cam"], same_pt + 1, c["edge_cam"][same_pt])))
    for key, i in (("cam_q", 6), ("cam_t", 13), ("cam_K", 2), ("cam_bf", 4)):
        for v in (np.nan, np.inf):
            refused(lib, mt, dict(c, **{key: at(c[key], i, v)}))
    zq = np.array(c["cam_q"], copy=True)
    zq[4] = 0.0
    refused(lib, mt, dict(c, cam_q=zq))
    for key in ("cam_q", "cam_t", "cam_K", "cam_bf", "world_pos", "edge_point", "edge_cam", "edge_obs", "edge_inv_sigma2"):
        refused(lib, mt, dict(c, **{key: None}, n_points=nP, n_edges=nE))
    for key in ("n_cams", "n_points", "n_edges"):
        refused(lib, mt, dict(c, **{key: -1}))
    for v in (-1, 2):
        refused(lib, mt, dict(c, robust=v))
    pool = F.MapPointPool(64, lib=lib)
    try:
        refused(lib, mt, dict({k: v for k, v in c.items() if k != "world_pos"}, pool=pool, slot=np.arange(nP, dtype=np.int32), n_points=nP),
                device=False)   # the host build reads host arrays only
    finally:
        pool.close()
