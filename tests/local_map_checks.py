"""Checks of the device-side Frame::isInFrustum loop and of the one-call Tracking::SearchLocalPoints (rgbl_frustum_cull,
rgbl_track_local_points, rgbl_map_points_*), shared by tests/test_local_map_emu.py (kernel sources under the SIMT emulator)
and tests/test_local_map_gpu.py (the product library on an MI355X).  The yardsticks are the numpy-float32 restatement of
the reference's lines (F.frustum_restatement, itself pinned to the reference's own code by tests/test_frustum_reference.py)
and the CPU oracle's search_local_points.  Everything is compared bit for bit; a NaN equals a NaN whatever its payload."""
import ctypes as C
import threading

import numpy as np

import frustum_golden as fg
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

MAP_KEYS = ("world_pos1", "normal1", "min_dist1", "max_dist1", "mp_desc1", "mp_observed1", "consider1")
_cache = {}


def base_case():
    """The golden case 'kitti' (tests/frustum_golden.py: make_local_map_case(600, 500, 71) + the edge points) and its restatement,
    computed once and never modified: callers copy."""
    if "kitti" not in _cache:
        c, _, _ = fg.make_case("kitti")
        _cache["kitti"] = (c, F.frustum_restatement(c))
    return _cache["kitti"]


def take_points(case, idx):
    """the case with the map points idx only"""
    return dict(case, **{k: np.ascontiguousarray(case[k][idx]) for k in MAP_KEYS if case.get(k) is not None})


def same(a, b):
    """bit-equal float arrays, NaN == NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_cull(got, want, what):
    (iv, rec, n), (wiv, wrec, _) = got, want
    assert np.array_equal(iv, wiv), "%s: mbTrackInView differs at %s" % (what, np.nonzero(iv != wiv)[0][:8])
    assert n == int(wiv.sum()), what
    for fld in ("proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
        assert same(rec[fld], wrec[fld]), "%s: %s differs at %s" % (what, fld, np.nonzero(rec[fld].view(np.uint32) != wrec[fld].view(np.uint32))[0][:8])
    assert np.array_equal(rec["level"], wrec["level"]), "%s: predicted level differs at %s" % (what, np.nonzero(rec["level"] != wrec["level"])[0][:8])


def pooled(lib, case, slots=None, capacity=None):
    """the case's map points in a pool (slot k of point k unless given); returns (pool, case in pool form without host arrays)"""
    n1 = len(case["world_pos1"])
    slots = np.arange(n1, dtype=np.int32) if slots is None else np.asarray(slots, np.int32)
    pool = F.MapPointPool(capacity or max(int(slots.max()) + 1 if n1 else 1, 1), lib=lib)
    if n1:
        pool.update(slots, case["world_pos1"], case["normal1"], case["min_dist1"], case["max_dist1"], case["mp_desc1"])
    hollow = {k: None for k in ("world_pos1", "normal1", "min_dist1", "max_dist1", "mp_desc1")}
    return pool, dict(case, pool=pool, slot1=slots, **hollow)


def expected_fused(case, th, nnratio):
    """restatement -> oracle: (in_view, rec, nToMatch, match2, nmatches)"""
    iv, rec, _ = F.frustum_restatement(case)
    n2 = len(case["kp2_xy"])
    if iv.sum() == 0 or n2 == 0:
        return iv, rec, int(iv.sum()), np.full(n2, -1, np.int32), 0
    m, nm = O.search_local_points(cases.local_points_from_cull(case, iv, rec), th, nnratio)
    return iv, rec, int(iv.sum()), m, nm


def assert_fused(got, want, what):
    assert_cull(got[:3], want[:3], what)
    assert got[4] == want[4] and np.array_equal(got[3], want[3]), "%s: matches differ (%d, expected %d)" % (what, got[4], want[4])


# ---- the cull against the restatement ------------------------------------------------------------------------------------
def check_cull_sizes(lib, sizes=(0, 1, 63, 64, 65, 257, 600)):
    """One block, a block boundary, several blocks; host arrays and pool; every exit of isInFrustum, every level, the edges."""
    case, (wiv, wrec, stage) = base_case()
    assert all((stage == s).mean() >= 0.05 for s in (1, 2, 3, 4)) and (stage == 5).mean() >= 0.3, np.bincount(stage)
    assert set(wrec["level"][stage == 5]) == set(range(8))
    mt = F.ORBmatcher(0.8, True, lib=lib)
    seen = 0
    for n1 in sizes:
        idx = np.arange(n1)
        c = take_points(case, idx)
        want = (wiv[idx], wrec[idx], None)
        assert_cull(mt.FrustumCull(c), want, "cull of %d points" % n1)
        if n1:
            pool, pc = pooled(lib, c)
            assert_cull(mt.FrustumCull(pc), want, "cull of %d pooled points" % n1)
            pool.close()
        seen += int(wiv[idx].sum())
    mt.close()
    return seen


# ---- the fused call -------------------------------------------------------------------------------------------------------
def check_fused(lib, th=3.0, nnratio=0.8):
    case, _ = base_case()
    mt = F.ORBmatcher(nnratio, True, lib=lib)
    got = mt.SearchLocalPoints(case, th)
    # (1) the cull alone, then rgbl_search_local_points on what it returned
    iv, rec, n = mt.FrustumCull(case)
    m, nm = mt.SearchLocalPoints(cases.local_points_from_cull(case, iv, rec), th)
    assert_fused(got, (iv, rec, n, m, nm), "fused call against cull + rgbl_search_local_points")
    # (2) the restatement, then the oracle
    assert_fused(got, expected_fused(case, th, nnratio), "fused call against restatement + oracle")
    assert got[4] > 60 and got[2] > 200, (got[4], got[2])
    # (3) the fixtures: what the reference's own isInFrustum / PredictScale left in the MapPoints, host-array and pool form
    assert fg.assert_matches_golden("kitti", lambda c: mt.SearchLocalPoints(c, th)[:2]) > 70
    pool, pc = pooled(lib, case)
    pooled_got = []
    assert fg.assert_matches_golden("kitti", lambda c: pooled_got.append(mt.SearchLocalPoints(dict(pc, consider1=c["consider1"]), th)) or pooled_got[0][:2]) > 70
    assert_fused(pooled_got[0], got, "pool form")
    pool.close()
    # the records are optional
    bare = mt.prepare_TrackLocalPoints(case, th, records=False)()
    assert bare[1] is None and bare[2] == got[2] and bare[4] == got[4] and np.array_equal(bare[3], got[3]) and np.array_equal(bare[0], got[0])
    mt.close()
    return got[4]


# ---- pool form against host-array form ------------------------------------------------------------------------------------
def check_pool(lib, th=3.0):
    case, _ = base_case()
    n1 = len(case["world_pos1"])
    rng = np.random.default_rng(5)
    mt = F.ORBmatcher(0.8, True, lib=lib)
    want = mt.SearchLocalPoints(case, th)
    # permuted and sparse slots
    slots = rng.permutation(4 * n1)[:n1].astype(np.int32)
    pool, pc = pooled(lib, case, slots, capacity=4 * n1)
    assert_fused(mt.SearchLocalPoints(pc, th), want, "pool with permuted, sparse slots")
    # a partial update: positions only, then the rest of two fields; the others stay
    moved = take_points(case, rng.permutation(n1))
    pool.update(slots, world_pos=moved["world_pos1"])
    pool.update(slots[:50], max_dist=moved["max_dist1"][:50], normal=moved["normal1"][:50])
    mixed = dict(case, world_pos1=moved["world_pos1"], max_dist1=case["max_dist1"].copy(), normal1=case["normal1"].copy())
    mixed["max_dist1"][:50] = moved["max_dist1"][:50]
    mixed["normal1"][:50] = moved["normal1"][:50]
    assert_fused(mt.SearchLocalPoints(pc, th), mt.SearchLocalPoints(mixed, th), "partial updates")
    assert_cull(mt.FrustumCull(pc), F.frustum_restatement(mixed), "partial updates against the restatement")
    # reserve keeps the contents, never shrinks, and new slots can be used
    pool.reserve(10 * n1 + 3)
    pool.reserve(5)
    assert pool.capacity() == 10 * n1 + 3
    assert_fused(mt.SearchLocalPoints(pc, th), mt.SearchLocalPoints(mixed, th), "after reserve")
    pool.update([10 * n1 + 2], world_pos=mixed["world_pos1"][7], normal=mixed["normal1"][7], min_dist=mixed["min_dist1"][7:8],
                max_dist=mixed["max_dist1"][7:8], desc=mixed["mp_desc1"][7])
    # repeated slots: a local map that lists a point twice; and one update that lists a slot twice keeps the last entry
    rep = rng.integers(0, n1, n1)
    rep[0] = 7
    pcr = dict(pc, slot1=np.where(np.arange(n1) == 0, 10 * n1 + 2, slots[rep]).astype(np.int32), consider1=case["consider1"][rep],
               mp_observed1=case["mp_observed1"][rep])
    assert_fused(mt.SearchLocalPoints(pcr, th), mt.SearchLocalPoints(take_points(mixed, rep), th), "repeated slots")
    a = take_points(dict(mixed, consider1=None), np.array([11, 12, 13]))
    pool.update([3, 9, 3], a["world_pos1"], a["normal1"], a["min_dist1"], a["max_dist1"], a["mp_desc1"])
    probe = dict(pc, slot1=np.array([3, 9], np.int32), consider1=None, mp_observed1=np.ones(2, np.uint8))
    assert_cull(mt.FrustumCull(probe), F.frustum_restatement(take_points(dict(mixed, consider1=None), np.array([13, 12]))),
                "a slot listed twice in one update")
    pool.close()
    mt.close()


# ---- special inputs -------------------------------------------------------------------------------------------------------
def check_special(lib, th=3.0, nnratio=0.8):
    case, (wiv, wrec, _) = base_case()
    n1, n2 = len(case["world_pos1"]), len(case["kp2_xy"])
    mt = F.ORBmatcher(nnratio, True, lib=lib)
    # bFarPoints: points in view beyond thFarPoints stay in view but are not matched
    near = expected_fused(dict(case, far_points=1), th, nnratio)
    assert int(((wrec["depth"] > case["th_far_points"]) & (wiv != 0)).sum()) > 20
    assert_fused(mt.SearchLocalPoints(dict(case, far_points=1), th), near, "bFarPoints")
    assert not np.array_equal(near[3], expected_fused(case, th, nnratio)[3])
    # consider1: NULL = every point
    everyone = dict(case, consider1=None)
    assert_fused(mt.SearchLocalPoints(everyone, th), expected_fused(everyone, th, nnratio), "consider1 NULL")
    # consider1 all zero: nothing in view, nToMatch == 0, no match, records as a point that is not considered
    nobody = dict(case, consider1=np.zeros(n1, np.uint8))
    got = mt.SearchLocalPoints(nobody, th)
    assert got[2] == 0 and got[4] == 0 and not got[0].any() and (got[3] == -1).all()
    assert_fused(got, expected_fused(nobody, th, nnratio), "consider1 all zero")
    # nToMatch == 0 found by the cull itself: every considered point is behind the camera
    back = dict(everyone, world_pos1=(2 * case["Ow"] - case["world_pos1"]).astype(np.float32))
    back["world_pos1"][wiv == 0] = case["world_pos1"][wiv == 0]
    back["consider1"] = wiv.copy()
    want = expected_fused(back, th, nnratio)
    assert want[2] == 0
    assert_fused(mt.SearchLocalPoints(back, th), want, "every point culled")
    # a frame that is resident on the device, with and without its own grid; its host arrays are not read
    for with_grid in (False, True):
        f2 = F.DeviceFrame(n2, lib=lib)
        f2.upload(case["desc2"], case["kp2_xy"], case["kp2_octave"], case["uright2"])
        if with_grid:
            f2.set_grid(case["grid"])
        hollow = dict(case, device2=f2, **{k: np.zeros_like(case[k]) for k in ("kp2_xy", "kp2_octave", "desc2", "uright2")})
        assert_fused(mt.SearchLocalPoints(hollow, th), expected_fused(case, th, nnratio), "resident frame")
        pool, pc = pooled(lib, hollow)
        assert_fused(mt.SearchLocalPoints(pc, th), expected_fused(case, th, nnratio), "resident frame, pooled points")
        pool.close()
        f2.close()
    # a frame without features
    empty = dict(case, **{k: case[k][:0] for k in ("kp2_xy", "kp2_octave", "desc2", "uright2", "blocked2")})
    got = mt.SearchLocalPoints(empty, th)
    assert_fused(got, expected_fused(empty, th, nnratio), "n2 == 0")
    assert got[2] == int(wiv.sum()) and len(got[3]) == 0
    # th == 1 (no factor), another ratio
    mt2 = F.ORBmatcher(0.7, True, lib=lib)
    assert_fused(mt2.SearchLocalPoints(case, 1.0), expected_fused(case, 1.0, 0.7), "th 1")
    # fewer levels than scale factors reach: the upper clamp moves
    low = dict(case, n_levels=5)
    assert_cull(mt.FrustumCull(low), F.frustum_restatement(low), "5 levels")
    mt2.close()
    mt.close()


# ---- error returns --------------------------------------------------------------------------------------------------------
def check_errors(lib):
    case, _ = base_case()
    case = take_points(case, np.arange(40))
    mt = F.ORBmatcher(0.8, True, lib=lib)
    pool, pc = pooled(lib, case, capacity=64)
    iv, rec, m2 = np.zeros(40, np.uint8), np.zeros(40, L.FRUSTUM_DTYPE), np.zeros(len(case["kp2_xy"]), np.int32)
    n, nm = C.c_int(0), C.c_int(0)

    def both(P):
        return (lib.rgbl_frustum_cull(mt.h, C.byref(P), L.ptr(iv), L.ptr(rec), C.byref(n)),
                lib.rgbl_track_local_points(mt.h, C.byref(P), L.ptr(iv), L.ptr(rec), C.byref(n), L.ptr(m2), C.byref(nm)))
    keep = []
    for bad in (-1, 64, 1 << 30):
        s = pc["slot1"].copy()
        s[17] = bad
        assert both(mt._track_local_input(dict(pc, slot1=s), 3.0, keep)) == (L.ERR_INVALID, L.ERR_INVALID)
        assert b"slot" in lib.rgbl_last_error()
    with np.testing.assert_raises(L.RgblError):
        pool.update([64], min_dist=np.ones(1, np.float32))
    with np.testing.assert_raises(L.RgblError):
        pool.update([3, -1], min_dist=np.ones(2, np.float32))
    P = mt._track_local_input(case, 3.0, keep)
    P.n1 = 1 << 20            # refused before any array is read
    assert both(P) == (L.ERR_INVALID, L.ERR_INVALID) and b"2^20" in lib.rgbl_last_error()
    for levels in (0, 17, -3):
        assert both(mt._track_local_input(dict(case, n_levels=levels), 3.0, keep)) == (L.ERR_INVALID, L.ERR_INVALID)
    P = mt._track_local_input(case, 3.0, keep)
    P.n2 = 65536
    assert lib.rgbl_track_local_points(mt.h, C.byref(P), L.ptr(iv), L.ptr(rec), C.byref(n), L.ptr(m2), C.byref(nm)) == L.ERR_INVALID
    P = mt._track_local_input(case, 3.0, keep)
    P.normal1 = None          # neither complete host arrays nor a pool
    assert both(P) == (L.ERR_INVALID, L.ERR_INVALID)
    P = mt._track_local_input(pc, 3.0, keep)
    P.slot1 = None
    assert both(P) == (L.ERR_INVALID, L.ERR_INVALID)
    assert lib.rgbl_frustum_cull(mt.h, None, L.ptr(iv), L.ptr(rec), C.byref(n)) == L.ERR_INVALID
    h = C.c_void_p()
    assert lib.rgbl_map_points_create(0, 0, C.byref(h)) == L.ERR_INVALID
    assert lib.rgbl_map_points_reserve(pool.h, -1) == L.ERR_INVALID
    # the handles still work
    assert_cull(mt.FrustumCull(pc), F.frustum_restatement(case), "after the error returns")
    pool.close()
    mt.close()


# ---- LocalMapping updates while Tracking searches ------------------------------------------------------------------------
def check_threads(lib, n=300, rounds=10, th=3.0):
    """One thread searches slots [0, n) of a pool while another rewrites slots [n, 2n) and grows the pool: every search must
    return what it returns single-threaded."""
    case, _ = base_case()
    case = take_points(case, np.arange(n))
    pool, pc = pooled(lib, case, capacity=2 * n)
    mt = F.ORBmatcher(0.8, True, lib=lib)
    want = mt.SearchLocalPoints(pc, th)
    want = tuple(np.copy(v) if isinstance(v, np.ndarray) else v for v in want)
    assert want[4] > 20
    errors = []

    def search():
        try:
            m = F.ORBmatcher(0.8, True, lib=lib)
            for r in range(rounds):
                assert_fused(m.SearchLocalPoints(pc, th), want, "search %d next to updates" % r)
            m.close()
        except Exception as ex:   # noqa: BLE001
            errors.append(ex)

    def update():
        try:
            rng = np.random.default_rng(3)
            other = np.arange(n, 2 * n, dtype=np.int32)
            for r in range(rounds):
                p = rng.permutation(n)
                pool.update(other, case["world_pos1"][p], case["normal1"][p], case["min_dist1"][p], case["max_dist1"][p], case["mp_desc1"][p])
                if r == rounds // 2:
                    pool.reserve(3 * n)
        except Exception as ex:   # noqa: BLE001
            errors.append(ex)
    ts = [threading.Thread(target=search), threading.Thread(target=update), threading.Thread(target=search)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert_fused(mt.SearchLocalPoints(pc, th), want, "after the threads")
    pool.close()
    mt.close()
