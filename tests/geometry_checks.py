"""The grid-walking ORBmatcher searches on cameras and pyramids other than KITTI's 1241 x 376 / (8, 1.2): one table of searches
(how to build a case, what the oracle says, how the library is called) shared by the oracle-only floor check, the emulator
tier, the GPU tier, the reference tier and the random shapes.  Every generated case must be worth its name: the oracle finds a
match for at least FLOOR of the points (SearchForInitialization: of the level-0 features) before any kernel is asked."""
import math

import numpy as np
import pytest

import parity_checks as pc
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

CAMERA_NAMES = cases.CAMERA_NAMES
PYRAMIDS = cases.PYRAMIDS
# every camera at (8, 1.2), the EuRoC camera at the other pyramids as well
MATRIX = [(c, PYRAMIDS[0]) for c in CAMERA_NAMES] + [("euroc_undistorted", p) for p in PYRAMIDS[1:]]
MATRIX_IDS = ["%s-%dx%g" % (c, p[0], p[1]) for c, p in MATRIX]
FLOOR = 0.05
_cameras = {}


def camera(name):
    if name not in _cameras:
        O.build()
        _cameras[name] = cases.named_camera(name, undistort=O.undistort_points)
    return _cameras[name]


def assert_floor(found, of, what):
    assert found >= math.ceil(FLOOR * of), "%s: the oracle matched %d of %d, the case checks next to nothing" % (what, found, of)


class Search:
    """make(cam, pyr, n1, n2, seed) -> case; oracle(case) -> (tuple of result arrays, matches found); run(lib, case) -> the same
    tuple from the library; of(case) -> what the floor is a share of."""

    def __init__(self, make, oracle, run, of=None, greedy=False):
        self.make, self.oracle, self.run, self.greedy = make, oracle, run, greedy
        self.of = of or (lambda case: len(case["valid1"] if "valid1" in case else case["has_mp1"]))


def _counted(result):
    """(match array, count) as the oracle's greedy searches return it -> (tuple of result arrays, count)"""
    m, n = result
    return (m,), n


def _with_matcher(ratio, ori, call):
    def run(lib, case):
        mt = F.ORBmatcher(ratio, ori, lib=lib)
        try:
            return call(mt, case)
        finally:
            mt.close()
    return run


def _projection(motion, th, mono, ori):
    return Search(lambda cam, pyr, n1, n2, seed: cases.make_projection_case(n1, n2, seed, motion, camera=cam, pyramid=pyr),
                  lambda case: _counted(O.search_by_projection(case, th, mono, ori)),
                  _with_matcher(0.9, ori, lambda mt, case: (mt.SearchByProjection(case, th, mono)[0],)), greedy=True)


def _kf_case(cam, pyr, n1, n2, seed):
    case = cases.make_relocalization_case(n1, n2, seed, camera=cam, pyramid=pyr)
    valid, level = cases.relocalization_prepass(case)
    ovalid, olevel = O.kf_projection_prepass(case)
    assert np.array_equal(valid, ovalid) and np.array_equal(level[valid != 0], olevel[valid != 0]), "relocalisation prepass"
    return dict(case, valid1=valid, level1=level)


def _fuse_case(cam, pyr, n1, n2, seed):
    case = cases.make_fuse_case(n1, n2, seed, camera=cam, pyramid=pyr)
    valid, level = cases.fuse_prepass(case)
    ovalid, olevel = O.fuse_prepass(case)
    assert np.array_equal(valid, ovalid) and np.array_equal(level[valid != 0], olevel[valid != 0]), "fuse prepass"
    return dict(case, valid1=valid, level1=level)


def _fuse_oracle(th):
    def oracle(case):
        best, n = O.fuse_search(case, th)
        assert n == int((best >= 0).sum())
        return (best,), n
    return oracle


def _fuse(th):
    return Search(_fuse_case, _fuse_oracle(th), _with_matcher(0.6, True, lambda mt, case: (mt.FuseSearch(case, th)[0],)))


def _project_search(th, form, max_dist):
    def oracle(case):
        best, dist = O.project_search(case, th, form, max_dist)
        return (best, dist), int((best >= 0).sum())
    return Search(lambda cam, pyr, n1, n2, seed: cases.make_project_search_case(n1, n2, seed, camera=cam, pyramid=pyr), oracle,
                  _with_matcher(0.75, True, lambda mt, case: tuple(mt.ProjectSearch(case, th, form, max_dist))))


def _projection_sim3(th, form, ratio):
    max_dist = int(np.floor(np.float32(50) * np.float32(ratio)))

    def make(cam, pyr, n1, n2, seed):
        case = cases.make_project_search_case(n1, n2, seed, camera=cam, pyramid=pyr)
        case["matched2"] = (np.random.default_rng(seed).random(n2) < 0.12).astype(np.uint8)
        return case

    def oracle(case):
        m, n = O.search_by_projection_sim3(case, case["matched2"], th, form, max_dist)
        free, _ = O.search_by_projection_sim3(case, np.zeros_like(case["matched2"]), th, form, max_dist)
        assert not np.array_equal(free, m)                       # the features matched on entry matter in this case
        return (m,), n
    return Search(make, oracle, _with_matcher(0.75, True, lambda mt, case: (mt.SearchByProjectionSim3(case, case["matched2"], th, form, max_dist)[0],)),
                  greedy=True)


def _initialization(window, ratio, ori):
    def oracle(case):
        m, prev, n = O.search_for_initialization(case, window, ratio, ori)
        return (m, prev.view(np.uint32)), n

    def call(mt, case):
        m, prev, _ = mt.SearchForInitialization(case, window)
        return m, prev.view(np.uint32)
    # n2 = n1: the second frame is the first one moved
    return Search(lambda cam, pyr, n1, n2, seed: cases.make_initialization_case(n1, seed, camera=cam, pyramid=pyr), oracle,
                  _with_matcher(ratio, ori, call), of=lambda case: int((case["kp1_octave"] == 0).sum()))


def _sim3(th):
    return Search(lambda cam, pyr, n1, n2, seed: cases.make_sim3_case(n1, seed, camera=cam, pyramid=pyr),
                  lambda case: _counted(pc.search_by_sim3(case, th, O.project_search)),
                  _with_matcher(0.75, True, lambda mt, case: (pc.search_by_sim3(case, th, mt.ProjectSearch)[0],)),
                  of=lambda case: len(case["prior12"]))


# th, ORBdist, ratios: what the reference's callers pass (Tracking.cc, LocalMapping.cc, LoopClosing.cc)
SEARCHES = {
    "projection": _projection("forward", 7.0, False, True),
    "projection_mono_wide": _projection("none", 15.0, True, False),
    "projection_keyframe": Search(_kf_case, lambda case: _counted(O.search_by_projection_kf(case, 10.0, 100, True)),
                                  _with_matcher(0.9, True, lambda mt, case: (mt.SearchByProjectionKeyFrame(case, 10.0, 100)[0],)), greedy=True),
    "local_points": Search(lambda cam, pyr, n1, n2, seed: cases.make_local_points_case(n1, n2, seed, camera=cam, pyramid=pyr),
                           lambda case: _counted(O.search_local_points(case, 3.0, 0.8)),
                           _with_matcher(0.8, True, lambda mt, case: (mt.SearchLocalPoints(case, 3.0)[0],)), greedy=True),
    "initialization": _initialization(100, 0.9, True),
    "fuse": _fuse(3.0),
    "project_search_form0": _project_search(4.0, 0, 50),          # Fuse(pKF, Scw, ...)
    "project_search_form1": _project_search(7.5, 1, 100),         # the directed searches of SearchBySim3
    "search_by_sim3": _sim3(7.5),
    "projection_sim3_form0": _projection_sim3(8, 0, 1.5),
    "projection_sim3_form2": _projection_sim3(30, 2, 1.0),
}
SEEDS = {name: 301 + 10 * i for i, name in enumerate(sorted(SEARCHES))}
# the same searches with drawn parameters (tests/fuzz_cases.py)
fuse, project_search, projection_sim3, initialization, sim3 = _fuse, _project_search, _projection_sim3, _initialization, _sim3
GREEDY_ON_FRAMES = ("projection", "projection_mono_wide", "projection_keyframe", "local_points")


def beyond_lds(name):
    """(n1, n2) at which search `name` leaves the LDS forms of its kernels (kGridLdsN2 = 8192 features; kResolveLdsN1 = 8192
    points, kResolveLdsN2 = 6144 features)"""
    if name in GREEDY_ON_FRAMES:
        return 8300, 6200          # the resolve kernels' global-memory form, k_proj_grid<true>
    if name in ("initialization", "search_by_sim3"):
        return 8300, 8300
    return 1200, 8300              # k_proj_grid<false> behind the best-only searches and SearchByProjection(pKF, Scw)


def check_search(lib, name, cam, pyr, n1, n2, seed=None):
    """One case of search `name`: the floor on the oracle's result, then (lib is not None) the library against the oracle, bit
    for bit.  Returns (matches found, what the floor is a share of)."""
    s = SEARCHES[name] if isinstance(name, str) else name
    name = name if isinstance(name, str) else "a drawn search"
    case = s.make(camera(cam) if isinstance(cam, str) else cam, pyr, n1, n2, SEEDS[name] if seed is None else seed)
    want, found = s.oracle(case)
    what = "%s on %s, pyramid %s, %d x %d" % (name, cam if isinstance(cam, str) else "a camera", pyr, n1, n2)
    assert_floor(found, s.of(case), what)
    if lib is not None:
        got = s.run(lib, case)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), "%s: result %d differs from the oracle's in %d places" % (what, k, int((np.asarray(g) != np.asarray(w)).sum()))
    return found, s.of(case)


# ---- 17 pyramid levels: one more than P.scale[] / inv_sigma2[] hold --------------------------------------------------------
def refusals(lib):
    """(entry point, thunk) pairs for the entry points of the grid searches (the ones that fill ProjDev::scale): each thunk calls
    its entry point with 17 pyramid levels and small, otherwise valid inputs.  (rgbl_map_points_refresh, the other reader of
    kProjMaxLevels, has its refusal in map_refresh_checks.check_errors.)"""
    pyr = (17, 1.1)
    mt = F.ORBmatcher(0.8, True, lib=lib)
    proj = cases.make_projection_case(40, 60, 3, pyramid=pyr)
    kf = _kf_case(None, pyr, 40, 60, 4)
    fuse = _fuse_case(None, pyr, 40, 60, 5)
    ps = cases.make_project_search_case(40, 60, 6, pyramid=pyr)
    lp = cases.make_local_points_case(40, 60, 7, pyramid=pyr)
    lm = cases.make_local_map_case(40, 60, 8)
    sf17 = proj["scale_factors"]
    lm = dict(lm, scale_factors=sf17, log_scale_factor=np.float32(np.log(np.float32(1.1))))
    assert len(sf17) == 17
    return mt, [("rgbl_search_by_projection", lambda: mt.SearchByProjection(proj, 7.0, False)),
                ("rgbl_search_by_projection_keyframe", lambda: mt.SearchByProjectionKeyFrame(kf, 10.0, 100)),
                ("rgbl_fuse_search", lambda: mt.FuseSearch(fuse, 3.0)),
                ("rgbl_project_search", lambda: mt.ProjectSearch(ps, 4.0, 0, 50)),
                ("rgbl_search_by_projection_sim3", lambda: mt.SearchByProjectionSim3(ps, np.zeros(60, np.uint8), 8, 0, 75)),
                ("rgbl_search_local_points", lambda: mt.SearchLocalPoints(lp, 3.0)),
                ("rgbl_frustum_cull", lambda: mt.FrustumCull(lm)),
                ("rgbl_track_local_points", lambda: mt.prepare_TrackLocalPoints(lm, 3.0)())]


def check_seventeen_levels_refused(lib):
    mt, calls = refusals(lib)
    try:
        for name, thunk in calls:
            with pytest.raises(L.RgblError) as e:
                thunk()
            assert e.value.code == L.ERR_INVALID, name
            assert "16 pyramid levels" in str(e.value), (name, str(e.value))
    finally:
        mt.close()


# ---- the same searches with the frame resident on the device, its grid built once for the camera's bounds --------------------
RESIDENT = ("projection", "projection_keyframe", "local_points", "fuse", "project_search_form0", "project_search_form1",
            "projection_sim3_form0", "projection_sim3_form2")


def check_resident_frames(lib, cam="euroc_undistorted", pyr=(8, 1.2), n1=1200, n2=1000):
    """rgbl_device_frame_set_grid for the camera's bounds, then every search that takes a resident frame: nobody runs the grid
    kernel, the candidate kernels initialise the holders themselves (init_taken); the host arrays of the frame are zeroed."""
    for name in RESIDENT:
        s = SEARCHES[name]
        case = s.make(camera(cam), pyr, n1, n2, SEEDS[name] + 1)
        want, found = s.oracle(case)
        assert_floor(found, s.of(case), "%s, resident frame" % name)
        f2 = F.DeviceFrame(n2, lib=lib)
        try:
            f2.upload(case["desc2"], case["kp2_xy"], case["kp2_octave"], case.get("uright2"))
            f2.set_grid(case["grid"])
            hollow = dict(case, device2=f2, **{k: np.zeros_like(case[k]) for k in ("kp2_xy", "kp2_octave", "desc2", "uright2") if k in case})
            got = s.run(lib, hollow)
            for k, (g, w) in enumerate(zip(got, want)):
                assert np.array_equal(g, w), "%s on a resident frame: result %d differs from the oracle's" % (name, k)
        finally:
            f2.close()
