"""Checks of rgbl_map_points_refresh (MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors for pool slots,
from observations in device-resident key frames) and rgbl_map_points_download, shared by tests/test_map_refresh_emu.py (kernel
sources under the SIMT emulator) and tests/test_map_refresh_gpu.py (the product library on an MI355X).  The yardsticks: for
normal and distances a numpy float32 restatement of src/MapPoint.cc:444-492, line by line (restate_normal), for the
descriptor the CPU oracle's distinctive_descriptors on rows gathered in numpy.  Everything is compared bit for bit (a NaN
equals a NaN whatever its payload), on the call's host outputs and on the pool read back with rgbl_map_points_download."""
import ctypes as C
import threading

import numpy as np

import local_map_checks as lc
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

LDS_ROWS = 128   # kRefreshLdsRows of csrc/matcher.hip: lists up to this length are selected in LDS, longer ones in the call's scratch
OBS_COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1, 300)
POINT_COUNTS = (0, 1, 63, 64, 65, 300)
KF_COUNTS = (1, 2, 40)
FIELDS = ("normal", "min_dist", "max_dist", "desc")
_cache = {}


# ---- the yardsticks -------------------------------------------------------------------------------------------------------
def restate_normal(case, pos):
    """src/MapPoint.cc:444-492 in numpy float32, one statement per line of the reference, every point at once (observation i of
    all points that have one is one step of the loop :447-466).  Returns (normal, mfMinDistance, mfMaxDistance, written)."""
    f = np.float32
    off, cnt = case["obs_off"][:-1].astype(np.int64), np.diff(case["obs_off"]).astype(np.int64)
    Pos = np.ascontiguousarray(pos, f).reshape(-1, 3)
    Ow = np.ascontiguousarray(case["kf_center"], f).reshape(-1, 3)
    scale = np.ascontiguousarray(case["scale_factors"], f)

    def norm(v):   # MatrixBase::norm: sqrt of the products summed left to right (csrc/frustum_math.h: fr_dot, fr_norm)
        s = v[:, 0] * v[:, 0]
        s = s + v[:, 1] * v[:, 1]
        s = s + v[:, 2] * v[:, 2]
        return np.sqrt(s)
    with np.errstate(all="ignore"):
        normal = np.zeros((len(Pos), 3), f)                        # :444-445 normal.setZero()
        n = np.zeros(len(Pos), np.int64)                           # :446
        for i in range(int(cnt.max()) if len(cnt) else 0):         # :447 the i-th observation, bad key frames included
            has = cnt > i
            Owi = Ow[case["obs_kf"][off[has] + i]]                 # :455 pKF->GetCameraCenter()
            normali = Pos[has] - Owi                               # :456
            normal[has] = normal[has] + normali / norm(normali)[:, None]   # :457
            n[has] += 1                                            # :458
        written = cnt > 0                                          # :441
        ref = np.where(written, case["ref_kf"], 0) if len(Ow) else np.zeros(len(Pos), np.int64)
        PC = Pos - (Ow[ref] if len(Ow) else 0)                     # :468
        dist = norm(PC)                                            # :469
        levelScaleFactor = scale[np.where(written, case["ref_level"], 0)]   # :485
        mfMaxDistance = dist * levelScaleFactor                    # :490
        mfMinDistance = mfMaxDistance / scale[int(case["n_levels"]) - 1]    # :491
        mNormalVector = normal / n.astype(f)[:, None]              # :492
    return mNormalVector.astype(f), mfMinDistance.astype(f), mfMaxDistance.astype(f), written


def restate_descriptor(case):
    """ComputeDistinctiveDescriptors: the rows of the key frames that are not bad, gathered here, through the oracle.
    Returns (descriptor or zeros, position of the winner in the point's own list or -1, written)."""
    n = len(case["slot"])
    start = np.concatenate([[0], np.cumsum(case["kf_n"])]).astype(np.int64)
    table = np.concatenate(case["kf_desc"]) if len(case["kf_desc"]) else np.zeros((0, 32), np.uint8)
    kf, feat = case["obs_kf"].astype(np.int64), case["obs_feat"].astype(np.int64)
    row_of_obs = table[start[kf] + feat] if len(kf) else np.zeros((0, 32), np.uint8)
    good = case["kf_bad"][kf] == 0 if len(kf) else np.zeros(0, bool)
    lists, where = [], []
    for p in range(n):
        b, e = int(case["obs_off"][p]), int(case["obs_off"][p + 1])
        idx = np.nonzero(good[b:e])[0]
        where.append(idx)
        lists.append(row_of_obs[b:e][idx])
    best = O.distinctive_descriptors(lists) if n else np.zeros(0, np.int32)
    desc, best_obs, written = np.zeros((n, 32), np.uint8), np.full(n, -1, np.int32), np.zeros(n, bool)
    for p in range(n):
        if len(where[p]):
            desc[p], best_obs[p], written[p] = lists[p][best[p]], where[p][best[p]], True
    return desc, best_obs, written


def expected(case, new_world_pos=None, do_normal=True, do_descriptor=True):
    """what the slots hold after the call, and what the call returns"""
    pos = case["world_pos"] if new_world_pos is None else np.ascontiguousarray(new_world_pos, np.float32)
    w = dict(world_pos=pos.copy(), normal=case["normal0"].copy(), min_dist=case["min_dist0"].copy(), max_dist=case["max_dist0"].copy(),
             desc=case["desc0"].copy(), best_obs=np.full(len(pos), -1, np.int32), status=np.zeros(len(pos), np.uint8))
    if do_normal:
        nv, mn, mx, wr = restate_normal(case, pos)
        w["normal"][wr], w["min_dist"][wr], w["max_dist"][wr] = nv[wr], mn[wr], mx[wr]
        w["status"] |= wr.astype(np.uint8)
    if do_descriptor:
        d, b, wr = restate_descriptor(case)
        w["desc"][wr], w["best_obs"][wr] = d[wr], b[wr]
        w["status"] |= wr.astype(np.uint8) << 1
    return w


def take_points(case, want, idx):
    """the case, and its expected values, with the points idx only (the key-frame side stays)"""
    idx = np.asarray(idx, np.int64)
    off = case["obs_off"].astype(np.int64)
    cnt = off[idx + 1] - off[idx]
    sel = np.concatenate([np.arange(off[p], off[p + 1]) for p in idx]) if len(idx) else np.zeros(0, np.int64)
    c = dict(case, slot=np.arange(len(idx), dtype=np.int32), obs_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32),
             obs_kf=case["obs_kf"][sel], obs_feat=case["obs_feat"][sel],
             **{k: case[k][idx] for k in ("world_pos", "normal0", "min_dist0", "max_dist0", "desc0", "ref_kf", "ref_level")})
    return c, {k: v[idx] for k, v in want.items()}


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def resident(lib, case):
    """the case's key frames as device frames"""
    return [F.DeviceFrame(len(d), lib=lib).upload(d, xy, o) for d, xy, o in zip(case["kf_desc"], case["kf_xy"], case["kf_octave"])]


def pooled(lib, case, capacity=None):
    """a pool that holds the points as they are before the refresh"""
    n = len(case["slot"])
    pool = F.MapPointPool(capacity or max(int(case["slot"].max()) + 1 if n else 1, 1), lib=lib)
    if n:
        pool.update(case["slot"], case["world_pos"], case["normal0"], case["min_dist0"], case["max_dist0"], case["desc0"])
    return pool


def assert_state(got, want, what, fields=FIELDS + ("world_pos",)):
    for k in fields:
        if k == "desc":
            assert np.array_equal(got[k], want[k]), "%s: desc differs at %s" % (what, np.nonzero((got[k] != want[k]).any(1))[0][:8])
        else:
            bad = np.nonzero(~((got[k].view(np.uint32) == want[k].view(np.uint32)) | (np.isnan(got[k]) & np.isnan(want[k]))))[0][:8]
            assert lc.same(got[k], want[k]), "%s: %s differs at %s: %s, expected %s" % (what, k, bad, got[k][bad[:2]], want[k][bad[:2]])


def refresh_and_compare(mt, pool, case, want, what):
    got = pool.refresh(mt, case)
    assert_state(got, want, what + " (returned)", FIELDS)
    assert np.array_equal(got["best_obs"], want["best_obs"]), "%s: best_obs differs at %s" % (what, np.nonzero(got["best_obs"] != want["best_obs"])[0][:8])
    assert np.array_equal(got["status"], want["status"]), "%s: status differs at %s" % (what, np.nonzero(got["status"] != want["status"])[0][:8])
    assert_state(pool.download(case["slot"]), want, what + " (pool)")
    return got


def close_all(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


# ---- 1. sizes ----------------------------------------------------------------------------------------------------------------
def sweep_case(n_kfs):
    """One case per key-frame count: max(POINT_COUNTS) points of every observation count, over key frames with differing feature
    counts; its expected values are computed once, never modified, and every (points, observations) combination is a slice.
    The observation on feature 0 of a frame is in every slice of one observation per point, the one on a frame's last feature
    in the slice of 300 points with 300 observations."""
    if n_kfs not in _cache:
        counts = np.repeat(OBS_COUNTS, max(POINT_COUNTS))
        case = cases.make_map_refresh_case(len(counts), n_kfs, seed=100 + n_kfs, obs_counts=counts, features=(40, 400))
        assert len(set(case["kf_n"].tolist())) == n_kfs and case["obs_feat"][0] == 0
        assert case["obs_feat"][-1] == case["kf_n"][case["obs_kf"][-1]] - 1
        _cache[n_kfs] = (case, expected(case))
    return _cache[n_kfs]


def check_sizes(lib, n_kfs, points=POINT_COUNTS, counts=OBS_COUNTS):
    """points x observations per point for one key-frame count: one wave / several / a grid of waves; empty lists, lists around the
    wave width and around the LDS capacity, one far beyond it.  Returns the number of (point, observation) pairs refreshed."""
    case, want = sweep_case(n_kfs)
    frames = resident(lib, case)
    mt = F.ORBmatcher(0.8, True, lib=lib)
    pairs = 0
    for o in counts:
        first = OBS_COUNTS.index(o) * max(POINT_COUNTS)
        for n in points:
            c, w = take_points(case, want, np.arange(first, first + n))
            pool = pooled(lib, c)
            refresh_and_compare(mt, pool, dict(c, kf_frames=frames), w, "%d points with %d observations, %d key frames" % (n, o, n_kfs))
            pairs += int(c["obs_off"][-1])
            pool.close()
    close_all(mt, frames)
    return pairs


# ---- 2. rules ----------------------------------------------------------------------------------------------------------------
def rules_case():
    if "rules" not in _cache:
        case = cases.make_map_refresh_case(90, 12, seed=7, features=(300, 500))
        case["obs_counts"] = np.diff(case["obs_off"])
        _cache["rules"] = case
    return {k: (v.copy() if isinstance(v, np.ndarray) else [a.copy() for a in v] if isinstance(v, list) else v) for k, v in _cache["rules"].items()}


def check_rules(lib):
    mt = F.ORBmatcher(0.8, True, lib=lib)
    rng = np.random.default_rng(11)
    case = rules_case()
    cnt = case["obs_counts"]
    # duplicate rows: the first minimum wins.  Point a: four equal rows; point b: one row of its own in front of three equal ones
    a, b = [int(p) for p in np.nonzero(cnt >= 4)[0][:2]]
    for p, rows in ((a, [0, 0, 0, 0]), (b, [1, 2, 2, 2])):
        n = int(cnt[p])
        src = rng.integers(0, 256, (3, 32), dtype=np.uint8)
        for i in range(n):
            o = int(case["obs_off"][p]) + i
            case["kf_desc"][case["obs_kf"][o]][case["obs_feat"][o]] = src[rows[min(i, 3)]]
    case["kf_bad"][:] = 0
    # bad key frames: left out of the descriptor, counted in the normal.  The first observation of point c is on a bad key frame
    c = int(np.nonzero(cnt >= 3)[0][5])
    case["kf_bad"][case["obs_kf"][case["obs_off"][c]]] = 1
    # the reference key frame is not an observer
    d = int(np.nonzero((cnt >= 2) & (cnt < 12))[0][7])
    case["ref_kf"][d] = np.setdiff1d(np.arange(12), case["obs_kf"][case["obs_off"][d]:case["obs_off"][d + 1]])[0]
    case["ref_level"][d] = case["kf_octave"][case["ref_kf"][d]][0]
    # permuted, sparse slots in a pool three times as large; the slots not listed hold other data
    n = len(case["slot"])
    case["slot"] = rng.permutation(3 * n)[:n].astype(np.int32)
    others = np.setdiff1d(np.arange(3 * n), case["slot"]).astype(np.int32)
    filler = cases.make_map_refresh_case(len(others), 1, seed=8, obs_counts=0)
    frames = resident(lib, case)
    run = dict(case, kf_frames=frames)

    def fresh():
        pool = pooled(lib, case, capacity=3 * n)
        pool.update(others, filler["world_pos"], filler["normal0"], filler["min_dist0"], filler["max_dist0"], filler["desc0"])
        return pool
    pool = fresh()
    before = pool.download(others)
    want = expected(case)
    got = refresh_and_compare(mt, pool, run, want, "rules")
    assert got["best_obs"][a] == 0 and got["best_obs"][b] == 1, (got["best_obs"][a], got["best_obs"][b])
    bad_obs = case["kf_bad"][case["obs_kf"]] != 0
    assert bad_obs[case["obs_off"][c]] and got["best_obs"][c] >= 1 and got["status"][c] == 3
    with_bad = np.add.reduceat(bad_obs, case["obs_off"][:-1][cnt > 0])
    assert (with_bad > 0).sum() >= 5
    assert (cnt == 0).any() and (got["status"][cnt == 0] == 0).all() and (got["status"][cnt > 0] & 1).all()
    assert_state(pool.download(others), before, "slots that are not listed")
    # do_normal only / do_descriptor only: the other half of the slots stays
    for flags in (dict(do_normal=1, do_descriptor=0), dict(do_normal=0, do_descriptor=1)):
        p2 = fresh()
        refresh_and_compare(mt, p2, dict(run, **flags), expected(case, **{k: bool(v) for k, v in flags.items()}), str(flags))
        p2.close()
    # do_normal only needs no resident key frame
    p2 = fresh()
    refresh_and_compare(mt, p2, dict(run, kf_frames=[None] * 12, do_descriptor=0), expected(case, do_descriptor=False), "no frames, do_normal only")
    p2.close()
    # every key frame bad: the descriptor stays, best_obs = -1; the normals are written all the same
    allbad = dict(case, kf_bad=np.ones(12, np.uint8))
    p2 = fresh()
    got = refresh_and_compare(mt, p2, dict(allbad, kf_frames=frames), expected(allbad), "every key frame bad")
    assert (got["best_obs"] == -1).all() and np.array_equal(got["desc"], case["desc0"]) and (got["status"][cnt > 0] == 1).all()
    p2.close()
    # kf_bad NULL: no key frame is bad
    nobad = dict(case, kf_bad=np.zeros(12, np.uint8))
    p2 = fresh()
    refresh_and_compare(mt, p2, dict(run, kf_bad=None), expected(nobad), "kf_bad NULL")
    p2.close()
    # world_pos with the call (SetWorldPos after bundle adjustment) = rgbl_map_points_update, then the call
    moved = (case["world_pos"] + rng.normal(0, 0.3, case["world_pos"].shape)).astype(np.float32)
    want = expected(case, new_world_pos=moved)
    assert not lc.same(want["normal"], expected(case)["normal"])
    p2, p3 = fresh(), fresh()
    refresh_and_compare(mt, p2, dict(run, new_world_pos=moved), want, "world_pos with the call")
    p3.update(case["slot"], world_pos=moved)
    refresh_and_compare(mt, p3, run, want, "world_pos through rgbl_map_points_update")
    everything = np.arange(3 * n, dtype=np.int32)
    assert_state(p2.download(everything), p3.download(everything), "both ways, the whole pool")
    # a second refresh changes nothing; no output struct, and only some outputs
    refresh_and_compare(mt, p2, run, want, "refreshed twice")
    p4 = fresh()
    keep = []
    P = p4.refresh_input(run, keep)
    assert lib.rgbl_map_points_refresh(mt.h, p4.h, C.byref(P), None) == L.RGBL_OK
    assert_state(p4.download(case["slot"]), expected(case), "no output struct")
    best = np.zeros(n, np.int32)
    out = L.MapRefreshOutput(None, None, None, L.ptr(best), None, None)
    assert lib.rgbl_map_points_refresh(mt.h, p4.h, C.byref(P), C.byref(out)) == L.RGBL_OK
    assert np.array_equal(best, expected(case)["best_obs"])
    close_all(pool, p2, p3, p4, mt, frames)


# ---- 3. wide range ----------------------------------------------------------------------------------------------------------
def check_wide_range(lib, n=2000):
    """Position magnitudes from 1e-3 to 1e4, as absolute positions and as offsets from an observing camera; one point exactly on a
    camera centre (0 / 0: NaN), one a float ulp away from it: the device's square root and division against the host's."""
    case = cases.make_map_refresh_case(n, 12, seed=21, obs_counts=8, features=(100, 200))
    rng = np.random.default_rng(22)
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mag = 10.0 ** rng.uniform(-3, 4, (n, 1))
    first_kf = case["obs_kf"][case["obs_off"][:-1]]
    near = (np.arange(n) % 2 == 1)[:, None]
    pos = np.where(near, case["kf_center"][first_kf].astype(np.float64) + d * mag, d * mag).astype(np.float32)
    last_kf = case["obs_kf"][case["obs_off"][1:] - 1]            # (not key frame 0, whose centre has x == 0)
    pos[3] = case["kf_center"][last_kf[3]]                        # on a camera centre that observes it ...
    case["ref_kf"][3] = last_kf[3]                                 # ... which is its reference key frame too: dist == 0
    pos[5] = case["kf_center"][last_kf[5]]
    pos[5, 0] = np.nextafter(pos[5, 0], np.float32(np.inf))       # a float ulp away
    case["world_pos"] = pos
    want = expected(case)
    assert np.isnan(want["normal"][3]).all() and want["max_dist"][3] == 0 and not np.isnan(want["normal"][5]).any()
    assert np.isnan(want["normal"]).any(1).sum() == 1
    lg = np.log10(np.abs(pos[np.abs(pos) > 0]))
    assert lg.min() < -3 and lg.max() > 3.5
    frames, pool, mt = resident(lib, case), pooled(lib, case), F.ORBmatcher(0.8, True, lib=lib)
    refresh_and_compare(mt, pool, dict(case, kf_frames=frames), want, "wide range")
    close_all(pool, mt, frames)


# ---- 4. consistency with what exists ----------------------------------------------------------------------------------------
def check_track_after_refresh(lib, th=3.0):
    """The local map of tests/local_map_checks.py, its normals, ranges and descriptors made by a refresh: rgbl_track_local_points
    on the pool equals the host-array form fed with the expected values."""
    base, _ = lc.base_case()
    n1 = len(base["world_pos1"])
    rng = np.random.default_rng(31)
    case = cases.make_map_refresh_case(n1, 10, seed=32, features=(300, 600), base_desc=base["mp_desc1"])
    case["world_pos"] = base["world_pos1"].copy()
    case["kf_center"] = (base["Ow"][None, :] + rng.normal(0, 0.4, (10, 3))).astype(np.float32)   # key frames around the camera
    case["scale_factors"], case["n_levels"] = np.ascontiguousarray(base["scale_factors"], np.float32), len(base["scale_factors"])
    case["ref_level"] = np.minimum(case["ref_level"], case["n_levels"] - 1)
    want = expected(case)
    frames, pool, mt = resident(lib, case), pooled(lib, case), F.ORBmatcher(0.8, True, lib=lib)
    refresh_and_compare(mt, pool, dict(case, kf_frames=frames), want, "local map")
    host = dict(base, normal1=want["normal"], min_dist1=want["min_dist"], max_dist1=want["max_dist"], mp_desc1=want["desc"])
    hollow = {k: None for k in ("world_pos1", "normal1", "min_dist1", "max_dist1", "mp_desc1")}
    fused = mt.SearchLocalPoints(host, th)
    fused = tuple(np.copy(v) if isinstance(v, np.ndarray) else v for v in fused)
    assert fused[2] > 100 and fused[4] > 10, (fused[2], fused[4])   # the comparison below is not about nothing
    lc.assert_fused(mt.SearchLocalPoints(dict(base, pool=pool, slot1=case["slot"], **hollow), th), fused, "track on the refreshed pool")
    lc.assert_fused(fused, lc.expected_fused(host, th, 0.8), "host-array form against restatement + oracle")
    close_all(pool, mt, frames)
    return fused[4]


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
def check_errors(lib):
    case = cases.make_map_refresh_case(40, 6, seed=41, features=(50, 90))
    frames, mt = resident(lib, case), F.ORBmatcher(0.8, True, lib=lib)
    pool = pooled(lib, case, capacity=64)
    everything = np.arange(64, dtype=np.int32)
    before = pool.download(everything)
    run = dict(case, kf_frames=frames)
    n = len(case["slot"])
    out_arrays = dict(normal=np.full((n, 3), 7, np.float32), best_obs=np.full(n, 7, np.int32))

    def refused(c, word=None, **kw):
        keep = []
        P = pool.refresh_input(c, keep)
        for k, v in kw.items():
            setattr(P, k, v)
        out = L.MapRefreshOutput(L.ptr(out_arrays["normal"]), None, None, L.ptr(out_arrays["best_obs"]), None, None)
        assert lib.rgbl_map_points_refresh(mt.h, pool.h, C.byref(P), C.byref(out)) == L.ERR_INVALID, (word, kw)
        if word:
            assert word in lib.rgbl_last_error(), lib.rgbl_last_error()
        assert_state(pool.download(everything), before, "after a refused call (%s)" % (word or kw))

    def poked(key, at, value):
        a = case[key].copy()
        a[at] = value
        return dict(run, **{key: a})
    for bad in (-1, 64, 1 << 30):
        refused(poked("slot", 17, bad), b"slot")
    refused(poked("slot", 17, case["slot"][3]), b"twice")
    last = len(case["obs_kf"]) - 1
    for bad in (-1, 6):
        refused(poked("obs_kf", last, bad), b"key frame")
        refused(poked("ref_kf", 5, bad), b"reference key frame")
    for bad in (-1, 8, 1 << 20):
        refused(poked("ref_level", 39, bad), b"level")
    o = int(case["obs_off"][20])
    for bad in (-1, int(case["kf_n"][case["obs_kf"][o]]), 1 << 30):
        refused(poked("obs_feat", o, bad), b"feature")
    some_missing = list(frames)
    some_missing[2] = None
    refused(dict(run, kf_frames=some_missing), b"not resident")
    down = case["obs_off"].copy()
    down[10] = down[9] - 1
    refused(dict(run, obs_off=down), b"ascend")
    shifted = case["obs_off"].copy()
    shifted[0] = 1
    refused(dict(run, obs_off=shifted), b"start at 0")
    many = dict(run, slot=case["slot"][:1], obs_off=np.array([0, 65536], np.int32), obs_kf=np.zeros(65536, np.int32),
                obs_feat=np.zeros(65536, np.int32), ref_kf=case["ref_kf"][:1], ref_level=case["ref_level"][:1])
    refused(many, b"65535")
    for levels in (0, 17, -3):
        refused(run, None, n_levels=levels)
    refused(run, None, n_points=-1)
    refused(run, None, slot=None)
    refused(run, None, obs_off=None)
    refused(run, None, obs_kf=None)
    refused(run, None, kf_center=None)
    refused(run, None, kf_frame=None)
    refused(run, None, scale_factors=None)
    keep = []
    P = pool.refresh_input(run, keep)
    assert lib.rgbl_map_points_refresh(None, pool.h, C.byref(P), None) == L.ERR_INVALID
    assert lib.rgbl_map_points_refresh(mt.h, None, C.byref(P), None) == L.ERR_INVALID
    assert lib.rgbl_map_points_refresh(mt.h, pool.h, None, None) == L.ERR_INVALID
    if lib.rgbl_device_count() > 1:   # a pool / a frame on another device than the matcher
        other_pool, other_frame = F.MapPointPool(64, device=1, lib=lib), F.DeviceFrame(90, device=1, lib=lib)
        assert lib.rgbl_map_points_refresh(mt.h, other_pool.h, C.byref(P), None) == L.ERR_INVALID
        refused(dict(run, kf_frames=[other_frame] + frames[1:]), b"device")
        other_mt = F.ORBmatcher(0.8, True, device=1, lib=lib)
        assert lib.rgbl_map_points_refresh(other_mt.h, pool.h, C.byref(P), None) == L.ERR_INVALID
        assert_state(pool.download(everything), before, "after a matcher on another device")
        close_all(other_pool, other_frame, other_mt)
    assert (out_arrays["normal"] == 7).all() and (out_arrays["best_obs"] == 7).all()
    with np.testing.assert_raises(L.RgblError):
        pool.download([64])
    with np.testing.assert_raises(L.RgblError):
        pool.download([0, -1])
    # no points: OK, whatever else the struct says
    P = L.MapRefreshInput()
    assert lib.rgbl_map_points_refresh(mt.h, pool.h, C.byref(P), None) == L.RGBL_OK
    assert len(pool.download([])["min_dist"]) == 0
    assert_state(pool.download(everything), before, "after n_points == 0")
    # the handles still work
    refresh_and_compare(mt, pool, run, expected(case), "after the error returns")
    close_all(pool, mt, frames)


# ---- 6. threads --------------------------------------------------------------------------------------------------------------
def check_threads(lib, n=150, rounds=6, th=3.0):
    """LocalMapping refreshes slots [0, n) while Tracking searches slots [n, 2n) of the same pool and a third thread rewrites
    slots [2n, 3n) and grows the pool: every refresh and every search returns what it returns single-threaded."""
    base, _ = lc.base_case()
    base = lc.take_points(base, np.arange(n))
    case = cases.make_map_refresh_case(n, 12, seed=51, features=(200, 300))
    frames, pool = resident(lib, case), pooled(lib, case, capacity=3 * n)
    tracked = np.arange(n, 2 * n, dtype=np.int32)
    pool.update(tracked, base["world_pos1"], base["normal1"], base["min_dist1"], base["max_dist1"], base["mp_desc1"])
    hollow = {k: None for k in ("world_pos1", "normal1", "min_dist1", "max_dist1", "mp_desc1")}
    pc = dict(base, pool=pool, slot1=tracked, **hollow)
    mt = F.ORBmatcher(0.8, True, lib=lib)
    want_search = tuple(np.copy(v) if isinstance(v, np.ndarray) else v for v in mt.SearchLocalPoints(pc, th))
    assert want_search[2] > 20
    want = expected(case)
    run = dict(case, kf_frames=frames)
    errors = []

    def guarded(body):
        def f():
            try:
                body()
            except Exception as ex:   # noqa: BLE001
                errors.append(ex)
        return f

    def refresh():
        m = F.ORBmatcher(0.8, True, lib=lib)
        for r in range(rounds):
            if r % 2 == 0:   # back to the state before, so that the next refresh has something to write
                pool.update(case["slot"], case["world_pos"], case["normal0"], case["min_dist0"], case["max_dist0"], case["desc0"])
            refresh_and_compare(m, pool, run, want, "refresh %d next to a search and updates" % r)
        m.close()

    def search():
        m = F.ORBmatcher(0.8, True, lib=lib)
        for r in range(rounds):
            lc.assert_fused(m.SearchLocalPoints(pc, th), want_search, "search %d next to refreshes" % r)
        m.close()

    def update():
        rng = np.random.default_rng(3)
        other = np.arange(2 * n, 3 * n, dtype=np.int32)
        for r in range(rounds):
            p = rng.permutation(n)
            pool.update(other, base["world_pos1"][p], base["normal1"][p], base["min_dist1"][p], base["max_dist1"][p], base["mp_desc1"][p])
            if r == rounds // 2:
                pool.reserve(4 * n)
    ts = [threading.Thread(target=guarded(f)) for f in (refresh, search, update)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    refresh_and_compare(mt, pool, run, want, "after the threads")
    lc.assert_fused(mt.SearchLocalPoints(pc, th), want_search, "search after the threads")
    close_all(pool, mt, frames)


# ---- 9. a map of KITTI size ---------------------------------------------------------------------------------------------------
def kitti_case(n_points=1500):
    """what tools/map_refresh_bench.py times: 40 key frames of 2 000 features, about 15 observations per point"""
    return cases.make_map_refresh_case(n_points, 40, seed=5, features=2000)


def check_kitti_size(lib):
    case = kitti_case()
    cnt = np.diff(case["obs_off"])
    assert 12 < cnt.mean() < 20 and cnt.max() > LDS_ROWS and (cnt == 0).any() and case["kf_bad"].any()
    want = expected(case)
    frames, pool, mt = resident(lib, case), pooled(lib, case), F.ORBmatcher(0.8, True, lib=lib)
    refresh_and_compare(mt, pool, dict(case, kf_frames=frames), want, "KITTI-size map")
    close_all(pool, mt, frames)
