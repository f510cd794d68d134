"""Every size limit of the library from both sides: the largest size an entry point accepts, with a result at the highest index
its packed field can hold, and one past it, refused.  The table of limits is in DESIGN.md ("Size limits"); the cases here are
shared by tests/test_limits_emu.py (kernel sources under the SIMT emulator) and tests/test_limits_gpu.py (the MI355X).

An at-limit case must be worth its name before any kernel is asked (as geometry_checks.assert_floor): (a) the reference matches
at least geometry_checks.FLOOR of what it is a share of, (b) its result refers to the last permitted index of the field and to at
least one index with the field's top bit set.  Where a generator does not give (b) by chance the case is built for it: a matched
row is swapped with the last one (swap_rows) and the reference runs again.

A refused call returns RGBL_ERR_INVALID with a message that names the limit, leaves every output as the caller filled it, and
the handle gives the right answer afterwards."""
import ctypes as C

import numpy as np
import pytest

import geometry_checks as gc
from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

N2_MAX = 65535                     # features of a frame: 16-bit feature indices (entry_feature, cell_items, s_ulist)
LAST2, TOP2 = N2_MAX - 1, 1 << 15
N1_MAX = (1 << 20) - 1             # map points of a call: 20-bit point indices in the resolve kernels' announcements
LAST1 = N1_MAX - 1
PATTERN = 0x5a

# the per-feature arrays of the second frame in the cases of orb_slam3_rgbl_amd/cases.py
FEATURE_KEYS = ("kp2_xy", "kp2_octave", "kp2_angle", "uright2", "desc2", "blocked2", "matched2", "occupied2")
# ... of the first frame of SearchForInitialization
FEATURE1_KEYS = ("kp1_octave", "kp1_angle", "desc1", "prev_matched")
SIDE_KEYS = ("kp_xy", "kp_octave", "desc", "mp_state", "mp_pos", "mp_normal", "mp_desc", "mp_min_dist", "mp_max_dist")


def swap_rows(case, keys, i, j):
    """rows i and j of every array of `case` named in `keys` change places (in place; an array under two names moves once)"""
    seen = set()
    for k in keys:
        a = case.get(k)
        if a is None or id(a) in seen:
            continue
        seen.add(id(a))
        a[[i, j]] = a[[j, i]]
    return case


def point_keys(case, n1):
    """the per-point arrays of a grid-search case: the names that end in 1 and have n1 rows"""
    return [k for k, v in case.items() if k.endswith("1") and isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == n1]


def swap_sim3_features(case, side, i, j):
    """features i and j of key frame `side` ("a1" / "a2") of a cases.make_sim3_case change places, with what names them"""
    swap_rows(case[side], SIDE_KEYS, i, j)
    prior, inv = case["prior12"], case["inv"]
    if side == "a1":
        prior[[i, j]] = prior[[j, i]]
        inv[[i, j]] = inv[[j, i]]
    else:
        for a in (prior, inv):
            at_i, at_j = a == i, a == j
            a[at_i], a[at_j] = j, i


# ---- 1. the grid searches ---------------------------------------------------------------------------------------------------
def features_named(name, case, want):
    """the second-frame feature indices the reference's result refers to"""
    r = want[0]
    if gc.SEARCHES[name].greedy:
        return np.nonzero(r >= 0)[0]                     # match2: one entry per feature
    if name == "search_by_sim3":
        return r[(r >= 0) & (r != case["prior12"])]      # the matches the call found, not the ones it was handed
    return r[r >= 0]                                     # a feature index per point (initialization: per first-frame feature)


def points_named(name, case, want):
    """the point (first-frame feature) indices the reference's result refers to"""
    r = want[0]
    if gc.SEARCHES[name].greedy:
        return r[r >= 0]
    if name == "search_by_sim3":
        return np.nonzero((r >= 0) & (r != case["prior12"]))[0]
    return np.nonzero(r >= 0)[0]


def _swap_feature(name, case, i, j):
    if name == "search_by_sim3":
        swap_sim3_features(case, "a2", i, j)
    else:
        swap_rows(case, FEATURE_KEYS, i, j)


def _swap_point(name, case, n1, i, j):
    if name == "search_by_sim3":
        swap_sim3_features(case, "a1", i, j)
    elif name == "initialization":
        swap_rows(case, FEATURE1_KEYS, i, j)
    else:
        swap_rows(case, point_keys(case, n1), i, j)


def search_case(name, cam, pyr, n1, n2, seed_offset=0):
    """(case, the reference's result) of search `name` with n2 features (initialization, search_by_sim3: n1 = n2 on both sides),
    conditions (a) and (b) asserted: the last feature and one with bit 15 set are named by the result; with n1 = n2 = N2_MAX the
    same for the first frame's features; with n1 > 65536 a point beyond 16 bits is."""
    s = gc.SEARCHES[name]
    case = s.make(gc.camera(cam), pyr, n1, n2, gc.SEEDS[name] + seed_offset)
    square = name in ("initialization", "search_by_sim3")
    rows1 = n2 if square else n1
    want, found = s.oracle(case)
    named = features_named(name, case, want)
    if n2 == N2_MAX and LAST2 not in named:
        _swap_feature(name, case, int(named[len(named) // 2]), LAST2)
        want, found = s.oracle(case)
    named1 = points_named(name, case, want)
    if square and n2 == N2_MAX and LAST2 not in named1:
        _swap_point(name, case, rows1, int(named1[len(named1) // 2]), LAST2)
        want, found = s.oracle(case)
    what = "%s on %s, pyramid %s, %d x %d" % (name, cam, pyr, n1, n2)
    gc.assert_floor(found, s.of(case), what)                                                      # (a)
    named, named1 = features_named(name, case, want), points_named(name, case, want)
    if n2 == N2_MAX:                                                                              # (b)
        assert LAST2 in named and ((named >= TOP2) & (named < LAST2)).any(), "%s: feature %d or bit 15 is not in the result" % (what, LAST2)
        if square:
            assert LAST2 in named1 and ((named1 >= TOP2) & (named1 < LAST2)).any(), "%s: first-frame feature %d is not matched" % (what, LAST2)
    if rows1 > 65536:
        assert (named1 >= 65536).any(), "%s: no matched point beyond 16 bits" % what
    return case, want


def same_result(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "%s: result %d differs from the reference's in %d places (first at %s)" % (
            what, k, int((np.asarray(g) != np.asarray(w)).sum()), np.nonzero(np.asarray(g) != np.asarray(w))[0][:4])


def check_search_at_limit(lib, name, cam="kitti", pyr=(8, 1.2), n1=600, n2=N2_MAX):
    case, want = search_case(name, cam, pyr, n1, n2)
    same_result(gc.SEARCHES[name].run(lib, case), want, "%s on %s %s, %d x %d" % (name, cam, pyr, n1, n2))


def check_resident_at_limit(lib, n1=600):
    """DeviceFrame(65535), the upload of 65535 features, set_grid, then every search that takes a resident frame with the frame's
    host arrays zeroed (geometry_checks.check_resident_frames at the capacity limit)"""
    f2 = F.DeviceFrame(N2_MAX, lib=lib)
    try:
        for name in gc.RESIDENT:
            case, want = search_case(name, "kitti", (8, 1.2), n1, N2_MAX, seed_offset=1)
            f2.upload(case["desc2"], case["kp2_xy"], case["kp2_octave"], case.get("uright2"))
            assert len(f2) == N2_MAX
            f2.set_grid(case["grid"])
            hollow = dict(case, device2=f2, **{k: np.zeros_like(case[k]) for k in ("kp2_xy", "kp2_octave", "desc2", "uright2") if k in case})
            same_result(gc.SEARCHES[name].run(lib, hollow), want, "%s on a resident frame of %d features" % (name, N2_MAX))
    finally:
        f2.close()


POINT_LIMIT_SEARCHES = ("projection", "local_points")


def point_limit_case(name, tail=3000, n2=2000):
    """N1_MAX points of which only the last `tail` are valid (the rest zero, so the work stays small); (a) over the tail, (b) the
    point LAST1 = 2^20 - 2 is matched."""
    s = gc.SEARCHES[name]
    small = s.make(gc.camera("kitti"), (8, 1.2), tail, n2, gc.SEEDS[name] + 2)
    keys = point_keys(small, tail)
    assert "valid1" in keys
    case = dict(small)
    for k in keys:
        full = np.zeros((N1_MAX,) + small[k].shape[1:], small[k].dtype)
        full[N1_MAX - tail:] = small[k]
        case[k] = full
    want, found = s.oracle(case)
    m = want[0]
    if LAST1 not in m:
        pts = m[m >= 0]
        swap_rows(case, keys, int(pts[len(pts) // 2]), LAST1)
        want, found = s.oracle(case)
    gc.assert_floor(found, tail, "%s with %d points, the last %d valid" % (name, N1_MAX, tail))
    m = want[0]
    assert LAST1 in m and (m[m >= 0] >= N1_MAX - tail).all()
    return case, want


def check_point_limit(lib, name):
    case, want = point_limit_case(name)
    same_result(gc.SEARCHES[name].run(lib, case), want, "%s with 2^20 - 1 points" % name)


# ---- refusals: the call's own closure gives the input block and the outputs ---------------------------------------------------
def closure_of(call):
    """the variables a frontend.prepare_* closure holds, by name"""
    return dict(zip(call.__code__.co_freevars, (c.cell_contents for c in call.__closure__)))


def assert_refused(call, say, **sizes):
    """`call` (a frontend.prepare_* closure over a small valid case) with the sizes of its input block overwritten: RGBL_ERR_INVALID,
    the message says `say`, the integer outputs keep the caller's pattern; then, the sizes restored, the call is what it was."""
    v = closure_of(call)
    P = v["pP"]._obj
    outs = [a for k, a in v.items() if isinstance(a, np.ndarray) and a.dtype in (np.int32, np.uint8) and k != "prev0"]
    assert outs
    good = tuple(np.copy(r) if isinstance(r, np.ndarray) else r for r in call())
    saved = {k: getattr(P, k) for k in sizes}
    for k, n in sizes.items():
        setattr(P, k, n)
    for a in outs:
        a.view(np.uint8)[...] = PATTERN
    with pytest.raises(L.RgblError) as e:
        call()
    assert e.value.code == L.ERR_INVALID and say in str(e.value), (sizes, str(e.value))
    for a in outs:
        assert (a.view(np.uint8) == PATTERN).all(), "a refused call wrote to an output (%s)" % (sizes,)
    for k, n in saved.items():
        setattr(P, k, n)
    again = call()
    for g, w in zip(again, good):
        assert np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w, "the call after the refused one differs"


def grid_search_calls(mt):
    """(entry point, closure over a small valid case, calls check_point_count) for the eight grid-search entry points,
    rgbl_search_for_initialization and rgbl_track_local_points"""
    proj = cases.make_projection_case(40, 60, 3)
    kf = gc._kf_case(None, None, 40, 60, 4)
    fuse = gc._fuse_case(None, None, 40, 60, 5)
    ps = cases.make_project_search_case(40, 60, 6)
    lp = cases.make_local_points_case(40, 60, 7)
    lm = cases.make_local_map_case(40, 60, 8)
    ini = cases.make_initialization_case(60, 9)
    return [("rgbl_search_by_projection", mt.prepare_SearchByProjection(proj, 7.0, False), True),
            ("rgbl_search_by_projection_keyframe", mt.prepare_SearchByProjectionKeyFrame(kf, 10.0, 100), True),
            ("rgbl_fuse_search", mt.prepare_FuseSearch(fuse, 3.0), False),
            ("rgbl_project_search", mt.prepare_ProjectSearch(ps, 4.0, 0, 50), False),
            ("rgbl_search_by_projection_sim3", mt.prepare_SearchByProjectionSim3(ps, np.zeros(60, np.uint8), 8, 0, 75), True),
            ("rgbl_search_local_points", mt.prepare_SearchLocalPoints(lp, 3.0), True),
            ("rgbl_frustum_cull", mt.prepare_FrustumCull(lm), True),
            ("rgbl_track_local_points", mt.prepare_TrackLocalPoints(lm, 3.0), True),
            ("rgbl_search_for_initialization", mt.prepare_SearchForInitialization(ini, 100), True)]


def check_grid_search_refusals(lib):
    """n2 = 65536 by every entry point that takes a frame; n1 = 2^20 by every one that announces points in 20 bits.  The sizes
    alone are overwritten: a call is refused before any array is read."""
    mt = F.ORBmatcher(0.8, True, lib=lib)
    try:
        for entry, call, twenty_bits in grid_search_calls(mt):
            if entry != "rgbl_frustum_cull":      # reads no frame
                assert_refused(call, "65535", n2=N2_MAX + 1)
            if twenty_bits:
                assert_refused(call, "2^20 - 1", n1=N1_MAX + 1)
    finally:
        mt.close()
    for cap in (N2_MAX + 1, 0):
        h = C.c_void_p()
        assert lib.rgbl_device_frame_create(0, cap, C.byref(h)) == L.ERR_INVALID and not h.value
        assert b"65535" in lib.rgbl_last_error()


# ---- 7. SearchByBoW: at most kBowBucket = 16384 features of the second set in one vocabulary node -------------------------------
BOW_BUCKET = 16384
SECOND_ROWS = ("desc", "xy", "octave", "angle", "uright", "has_mp")


def _bow_forms():
    """(what, nnratio, second set is a two-camera frame, reference(first, second, n_left), call(matcher, first, second, n_left),
    (positions, owners) of a result): the three overloads"""
    def per_second(m):       # one entry per second-set feature: the first-set feature it got
        pos = np.nonzero(m >= 0)[0]
        return pos, m[pos]

    def per_first(m):        # one entry per first-set feature: the second-set feature it took
        own = np.nonzero(m >= 0)[0]
        return m[own], own
    return [("SearchByBoW(KF, F)", 0.7, False, lambda a, b, nl: O.search_by_bow(a, b, 0.7, True),
             lambda mt, a, b, nl: mt.prepare_SearchByBoW(a, b), per_second),
            ("SearchByBoW(KF, two-camera F)", 0.7, True, lambda a, b, nl: O.search_by_bow(a, b, 0.7, True, n_left=nl),
             lambda mt, a, b, nl: mt.prepare_SearchByBoW(a, b, nl), per_second),
            ("SearchByBoW(KF, KF)", 0.75, False, lambda a, b, nl: O.search_by_bow_kf(a, b, 0.75, True),
             lambda mt, a, b, nl: mt.prepare_SearchByBoWKeyFrames(a, b), per_first)]


def bow_bucket_case(form, bucket=BOW_BUCKET, short=64, seed=5):
    """One vocabulary node that holds `bucket` features of the second set (parity_checks.make_bucket_case / make_bucket_rig_case) and
    `short` of the first: the ones the reference matches to the highest bucket positions, to those on both sides of the register
    trips' end at 256, and to positions spread over the bucket.  The last position holds a matched feature: if the reference left it
    without a match, the feature of the highest matched position changes places with it.
    Returns (first set, second set, n_left, the reference's result)."""
    import parity_checks as pc
    what, _, rig, reference, _, named = form
    if rig:
        first, second, n_left = pc.make_bucket_rig_case(seed, (bucket,))
    else:
        first, second, *_ = pc.make_bucket_case(seed, (bucket,))
        n_left = -1
    first = dict(first, has_mp=np.ones(len(first["desc"]), np.uint8))
    second = dict(second, has_mp=np.ones(bucket, np.uint8))
    assert np.array_equal(second["node_feat"], np.arange(bucket)) and len(second["desc"]) == bucket   # bucket position = feature index
    pos, own = named(reference(first, second, n_left)[0])
    order = np.argsort(pos)
    pos, own = pos[order], own[order]
    near = np.argsort(np.abs(pos - 256), kind="stable")[:6]
    chosen = list(range(len(pos) - 4, len(pos))) + near.tolist() + list(range(0, len(pos), max(len(pos) // short, 1)))
    keep = []
    for k in chosen:
        if int(own[k]) not in keep and len(keep) < short:
            keep.append(int(own[k]))
    first = dict(first, node_feat=np.sort(np.array(keep, np.int32)), node_off=np.array([0, len(keep)], np.int32))
    want = reference(first, second, n_left)
    pos, _ = named(want[0])
    if bucket - 1 not in pos:
        swap_rows(second, SECOND_ROWS, bucket - 1, int(pos.max()))
        want = reference(first, second, n_left)
        pos, _ = named(want[0])
    gc.assert_floor(len(pos), len(keep), what)                                                                       # (a)
    assert bucket - 1 in pos and ((pos >= 256) & (pos < bucket - 1)).any() and (pos < 256).any(), "%s: position %d is not matched" % (what, bucket - 1)
    assert ((pos >= bucket // 2) & (pos < bucket - 1)).any()                                                         # (b)
    return first, second, n_left, want


def check_bow_at_limit(lib, which, short=64):
    form = _bow_forms()[which]
    first, second, n_left, (om, onm) = bow_bucket_case(form, short=short)
    mt = F.ORBmatcher(form[1], True, lib=lib)
    m, nm = form[4](mt, first, second, n_left)()
    assert nm == onm and np.array_equal(m, om), "%s, a bucket of %d" % (form[0], BOW_BUCKET)
    mt.close()


def check_bow_refused(lib):
    """a bucket of 16385 by each overload: refused before the output is written; then a valid call on the same handle"""
    for form in _bow_forms():
        import parity_checks as pc
        first, second, *rest = pc.make_bucket_rig_case(3, (BOW_BUCKET + 1,)) if form[2] else pc.make_bucket_case(3, (BOW_BUCKET + 1,))
        n_left = rest[0] if form[2] else -1
        first = dict(first, has_mp=np.ones(len(first["desc"]), np.uint8), node_feat=first["node_feat"][:8], node_off=np.array([0, 8], np.int32))
        second = dict(second, has_mp=np.ones(BOW_BUCKET + 1, np.uint8))
        mt = F.ORBmatcher(form[1], True, lib=lib)
        call = form[4](mt, first, second, n_left)
        out = closure_of(call)["m"]
        out[:] = 0x5a5a5a5a
        with pytest.raises(L.RgblError) as e:
            call()
        assert e.value.code == L.ERR_INVALID and str(BOW_BUCKET) in str(e.value), str(e.value)
        assert (out == 0x5a5a5a5a).all(), "%s: a refused call wrote to its output" % form[0]
        a, b, nl, (om, onm) = bow_bucket_case(form, bucket=300, short=40)
        m, nm = form[4](mt, a, b, nl)()
        assert nm == onm > 0 and np.array_equal(m, om), "%s after a refused call" % form[0]
        mt.close()


# ---- 11. KeyFrameDatabase: at most 65535 queries per call (one grid row each) ---------------------------------------------------
KFDB_QUERIES = 65535


def check_kfdb_query_limit(lib, n_words=24):
    """KFDB_QUERIES one-word queries against a small database in one rgbl_kfdb_query_batch; the reference is kfdb_ref, once per
    distinct word.  The last query (65534) and one with bit 15 set have candidates, and their neighbours have none."""
    import kfdb_checks as kk
    from orb_slam3_rgbl_amd import kfdb_cases as kc
    db = kc.make_database(40, 30, 600, seed=17)
    dev, ref = kk.fill(lib, db)
    stored = np.unique(np.concatenate([e["word_id"] for e in db["entries"]]))
    absent = np.setdiff1d(np.arange(600, dtype=np.uint32), stored)
    assert len(stored) >= n_words and len(absent) >= 2
    words = np.concatenate([stored[:: max(len(stored) // n_words, 1)][:n_words], absent[:2]]).astype(np.uint32)
    word_of = np.arange(KFDB_QUERIES) % len(words)
    word_of[KFDB_QUERIES - 1], word_of[KFDB_QUERIES - 2] = 0, len(words) - 1       # the last query finds key frames, the one before none
    word_of[1 << 15], word_of[(1 << 15) - 1] = 1, len(words) - 2
    one = np.array([1.0])
    exp = [ref.sharing(kk.Ids.next(), words[k:k + 1], one) for k in range(len(words))]
    assert len(exp[0]["kf"]) > 0 and exp[0]["scored"].any() and len(exp[1]["kf"]) > 0 and len(exp[-1]["kf"]) == 0 and len(exp[-2]["kf"]) == 0
    assert sum(len(e["kf"]) > 0 for e in exp) >= gc.FLOOR * len(exp)
    got = dev.query_batch([dict(word_id=words[k:k + 1], word_val=one) for k in word_of])
    assert len(got) == KFDB_QUERIES
    for q, k in enumerate(word_of):
        kk.assert_same(got[q], exp[k], "query %d of %d" % (q, KFDB_QUERIES))
    # one more: refused, nothing written; the handle answers afterwards
    call = dev.prepare_query_batch([dict(word_id=words[k:k + 1], word_val=one) for k in np.arange(KFDB_QUERIES + 1) % len(words)])
    outs = [a for a in closure_of(call).values() if isinstance(a, np.ndarray)]
    for a in outs:
        a.view(np.uint8)[...] = PATTERN
    with pytest.raises(L.RgblError) as e:
        call()
    assert e.value.code == L.ERR_INVALID and "65535" in str(e.value), str(e.value)
    assert all((a.view(np.uint8) == PATTERN).all() for a in outs), "a refused call wrote to an output"
    kk.assert_same(dev.query(words[:1], one), exp[0], "after the refused call")
    dev.close()


# ---- 8. depth module: the index map's entry is generation << 20 | point index + 1 (kIdxBits) ------------------------------------
IDX_FIELD = (1 << 20) - 1          # kIdxMask of csrc/depth.hip: `(uint32_t)n < kIdxMask` takes the indexed path
DEPTH_COUNTS = (IDX_FIELD - 1, IDX_FIELD, IDX_FIELD + 1)      # the largest count on the indexed path, the first two off it


def check_depth_index_limit(lib, w=310, h=94, n_kp=1500):
    """Scans of 2^20 - 2, 2^20 - 1 and 2^20 points over a 310 x 94 image (a few dozen points per pixel: the last one wins), inverse
    dilation, against the oracle bit for bit: without the maps (the indexed path for the first count, several calls in a row so
    that generation bits sit above a full index field), with them, and without them again."""
    import os

    import parity_checks as pc
    from orb_slam3_rgbl_amd import synth
    K = synth.KITTI_K.copy()
    K[0, 2], K[1, 2] = w / 2.0, h / 2.0
    K[0, 0] = K[1, 1] = 718.856 * w / synth.KITTI_W
    proj = F.projection_matrix(K, synth.KITTI_TR, lib)
    scan = synth.lidar_scan(3, n_az=16400)
    assert scan.shape[1] >= DEPTH_COUNTS[-1]
    rng = np.random.default_rng(23)
    kp = np.stack([rng.uniform(19, w - 20, n_kp), rng.uniform(19, h - 20, n_kp)], 1).astype(np.float32)
    kp[: n_kp // 2] = np.floor(kp[: n_kp // 2])
    kpun = kp.copy()
    kpun[:, 0] += rng.uniform(-1, 1, n_kp).astype(np.float32)
    P = O.make_depth_params(proj)
    saved = os.environ.pop("RGBL_DEPTH_MAX_GEN", None)       # read when the handle is created: the full generation range
    try:
        dm = F.DepthModule(proj, w, h, max_points=DEPTH_COUNTS[-1], max_keypoints=n_kp, lib=lib)
    finally:
        if saved is not None:
            os.environ["RGBL_DEPTH_MAX_GEN"] = saved
    try:
        for n in DEPTH_COUNTS:
            cloud = np.ascontiguousarray(scan[:, :n])
            # the last point lies on the ray of an earlier one that falls into the image, a little nearer
            seen = next(i for i in range(n) if (O.depth(P, np.ascontiguousarray(cloud[:, i:i + 1]), w, h, kp[:1], kpun[:1, 0])[2] > 0).any())
            cloud[:3, n - 1] = cloud[:3, seen] * np.float32(0.98)
            d, ur, raw, proc = O.depth(P, cloud, w, h, kp, kpun[:, 0])
            what = "%d points" % n
            # (a) the keypoints get depths; (b) the order of the points decides pixels, and the last point decides one
            gc.assert_floor(int((d > 0).sum()), n_kp, what)
            assert not np.array_equal(pc.bits(raw), pc.bits(O.depth(P, np.ascontiguousarray(cloud[:, ::-1]), w, h, kp, kpun[:, 0])[2])), what
            assert not np.array_equal(pc.bits(raw), pc.bits(O.depth(P, np.ascontiguousarray(cloud[:, :n - 1]), w, h, kp, kpun[:, 0])[2])), what
            for k in range(3):
                dm.CalculateDepthFromPcd(kp, kpun, cloud, w, h, want_maps=False)
                assert np.array_equal(pc.bits(dm.mvDepth), pc.bits(d)), "%s, call %d without the maps: mvDepth" % (what, k)
                assert np.array_equal(pc.bits(dm.mvuRight), pc.bits(ur)), "%s, call %d without the maps: mvuRight" % (what, k)
            dm.CalculateDepthFromPcd(kp, kpun, cloud, w, h, want_maps=True)
            assert np.array_equal(pc.bits(dm.RawDepthMap), pc.bits(raw)), "%s: RawDepthMap" % what
            assert np.array_equal(np.isnan(dm.ProcessedDepthMap), np.isnan(proc)), what
            assert np.array_equal(pc.bits(np.nan_to_num(dm.ProcessedDepthMap)), pc.bits(np.nan_to_num(proc))), "%s: ProcessedDepthMap" % what
            assert np.array_equal(pc.bits(dm.mvDepth), pc.bits(d)) and np.array_equal(pc.bits(dm.mvuRight), pc.bits(ur)), "%s with the maps" % what
            dm.CalculateDepthFromPcd(kp, kpun, cloud, w, h, want_maps=False)
            assert np.array_equal(pc.bits(dm.mvDepth), pc.bits(d)) and np.array_equal(pc.bits(dm.mvuRight), pc.bits(ur)), "%s after the maps" % what
    finally:
        dm.close()


# ---- 6. ComputeDistinctiveDescriptors / the map refresh: at most 65535 observations of a point (median << 16 | row) --------------
# oracle_py.distinctive_descriptors is quadratic in time and memory (73 s for 32769 rows): at the limit the reference is a
# multiplicity model, held to the oracle at sizes the oracle can do (tests/test_limits_emu.py).
OBS_MAX = 65535


def multiplicity_winner(values, value_of_row):
    """MapPoint::ComputeDistinctiveDescriptors for rows drawn from a few distinct descriptors: row i has the descriptor
    values[value_of_row[i]].  The sorted distances of a row are those of its value to every value, each as often as that value
    occurs; the median is the one at index (size_t)(0.5 * (N - 1)); the first row whose value has the least median wins."""
    values, value_of_row = np.asarray(values, np.uint8), np.asarray(value_of_row, np.int64)
    n, k = len(value_of_row), len(values)
    table = np.unpackbits(values[:, None, :] ^ values[None, :, :], axis=2).sum(2)        # k x k Hamming distances
    count = np.bincount(value_of_row, minlength=k)
    at = int(0.5 * (n - 1))
    median = np.empty(k, np.int64)
    for v in range(k):
        order = np.argsort(table[v], kind="stable")
        median[v] = table[v][order][np.searchsorted(np.cumsum(count[order]), at, side="right")]
    present = count > 0
    least = median[present].min()
    return int(np.nonzero(present[value_of_row] & (median[value_of_row] == least))[0][0])


def multiplicity_rows(n, seed, k=16, ties=False, winner_from=None, winner_only_at=None):
    """(values, value_of_row) for n rows of k distinct descriptors around a common ancestor.  ties: two values are equal bit for bit
    (their rows tie, the first wins) and two more lie symmetrically.  winner_from: the rows of the winning value start there, the
    rows before it are the other values'; winner_only_at: the winning value has this one row."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    flips = rng.random((k, 256)) < rng.uniform(0.03, 0.25, (k, 1))
    flips[0] = False                                              # the ancestor itself: the value nearest to all the others
    values = base ^ np.packbits(flips, axis=1, bitorder="little")
    if ties:
        values[3] = values[0]
        values[5] = values[4]
    if winner_from is None and winner_only_at is None:
        return values, rng.choice(k, n, p=rng.dirichlet(np.ones(k)))
    others = rng.integers(1, k, n)
    if ties:
        others[others == 3] = 2                                   # the twin of the winning value would win at its first row
    if winner_only_at is not None:
        others[winner_only_at] = 0
    else:
        others[winner_from:] = np.where(rng.random(n - winner_from) < 0.3, 0, others[winner_from:])
        others[winner_from] = 0
    return values, others


def check_multiplicity_model(sizes=(600, 2049), seeds=range(6)):
    """the model against oracle_py.distinctive_descriptors: random multiplicities, ties between values, the directed layouts"""
    lists, want = [], []
    for n in sizes:
        for seed in seeds:
            for kw in (dict(), dict(ties=True), dict(winner_from=n // 2), dict(winner_only_at=n - 1), dict(ties=True, winner_from=n // 2 + 1)):
                values, rows = multiplicity_rows(n, 100 * n + seed, **kw)
                lists.append(values[rows])
                want.append(multiplicity_winner(values, rows))
    got = O.distinctive_descriptors(lists)
    assert np.array_equal(got, np.array(want)), np.nonzero(got != np.array(want))[0]
    return len(lists)


OBS_TESTED = 32769      # the smallest count with bit 15 set: a point of 65535 observations keeps its one wave busy for a minute


def distinctive_limit_lists(n=OBS_TESTED):
    """(descriptor lists, expected winners): two points with n observations next to a few ordinary ones, in one call (one wave
    each, side by side).  The winning value of the first occurs from a row with bit 15 set on (n = 32769: its only row), that of the second only
    in the last row.  Condition (b) holds by construction and is asserted on the model's answer."""
    small = [multiplicity_rows(m, 7 + m) for m in (1, 5, 64, 130)]
    first_from = min(32768 + 5, n - 1)
    big = [multiplicity_rows(n, 31, winner_from=first_from), multiplicity_rows(n, 37, winner_only_at=n - 1)]
    want = np.array([multiplicity_winner(v, r) for v, r in big + small], np.int32)
    assert want[0] == first_from >= 32768 and want[1] == n - 1 >= 32768, want[:2]
    return [v[r] for v, r in big + small], want


def check_distinctive_limit(lib, n=OBS_TESTED):
    """rgbl_distinctive_descriptors on points with n observations"""
    mt = F.ORBmatcher(0.6, True, lib=lib)
    lists, want = distinctive_limit_lists(n)
    got = mt.ComputeDistinctiveDescriptors(lists)
    assert np.array_equal(got, want), "BestIdx %s, expected %s" % (got, want)
    mt.close()


def check_distinctive_refused(lib):
    """65536 observations of one point: RGBL_ERR_INVALID that names 65535, `best` untouched, the handle works afterwards"""
    mt = F.ORBmatcher(0.6, True, lib=lib)
    desc = np.zeros((OBS_MAX + 1 + 3, 32), np.uint8)
    off = np.array([0, 3, OBS_MAX + 1 + 3], np.int32)
    best = np.full(2, 0x5a5a5a5a, np.int32)
    rc = lib.rgbl_distinctive_descriptors(mt.h, L.ptr(desc), L.ptr(off), 2, L.ptr(best))
    assert rc == L.ERR_INVALID and b"65535" in lib.rgbl_last_error(), (rc, lib.rgbl_last_error())
    assert (best == 0x5a5a5a5a).all()
    values, rows = multiplicity_rows(130, 3)
    assert mt.ComputeDistinctiveDescriptors([values[rows]])[0] == multiplicity_winner(values, rows)
    mt.close()


def check_refresh_limit(lib, n=OBS_TESTED):
    """rgbl_map_points_refresh with a point of n observations: the descriptor rule on rows gathered from resident key frames (the
    scratch form of k_map_refresh_desc), best_obs = the winning observation's position, 16 bits wide in the kernel's key"""
    import map_refresh_checks as mr
    lists, want = distinctive_limit_lists(n)
    counts = np.array([len(d) for d in lists])
    n_kfs = 8
    per_kf = -(-int(counts.sum()) // n_kfs) + 1
    case = cases.make_map_refresh_case(len(lists), n_kfs, seed=9, obs_counts=counts, features=per_kf)
    # observation o of the whole list sits on key frame o % n_kfs, feature o // n_kfs, which holds its row
    o = np.arange(int(counts.sum()))
    case["obs_kf"], case["obs_feat"] = (o % n_kfs).astype(np.int32), (o // n_kfs).astype(np.int32)
    rows = np.concatenate(lists)
    for k in range(n_kfs):
        case["kf_desc"][k][: len(rows[k::n_kfs])] = rows[k::n_kfs]
    case["kf_bad"][:] = 0
    case["ref_kf"][:] = 0
    exp = mr.expected(case, do_descriptor=False)
    exp["best_obs"], exp["desc"] = want.copy(), np.stack([d[w] for d, w in zip(lists, want)])
    exp["status"] |= 2
    frames, pool, mt = mr.resident(lib, case), mr.pooled(lib, case), F.ORBmatcher(0.8, True, lib=lib)
    mr.refresh_and_compare(mt, pool, dict(case, kf_frames=frames), exp, "refresh of points with %d observations" % n)
    mr.close_all(pool, mt, frames)


# ---- 9. extractor: images of at most 4096 x 4096 (cnt << 28 | x0 << 16 | pos), node lists of at most 65535 entries ----------------
SIDE_MAX = 4096


def check_extractor_width_limit(lib, nfeatures, w=SIDE_MAX, h=360):
    """A 4096 x 360 image on 8 levels (288 rows would give level 3 seventeen quad-tree roots, one more than the library takes):
    12 roots on level 0, 16 on level 7, node x0 up to about 4000 inside the quad-tree's sort key.  Keypoints, descriptors and
    every stage against the oracle (parity_checks.check_extractor)."""
    import parity_checks as pc
    from orb_slam3_rgbl_amd import synth
    okps = O.Extractor(nfeatures, 1.2, 8, 12, 7)(synth.Sequence(0, w, h, n_frames=1).frame(0))[0]
    gc.assert_floor(len(okps), nfeatures, "%d x %d, %d features" % (w, h, nfeatures))                                 # (a)
    level0 = okps["x"][okps["octave"] == 0]
    assert level0.max() >= w - 96 and ((level0 >= 2048) & (level0 < w - 96)).any(), level0.max()                       # (b)
    sizes = [(2 * round(w / 1.2 ** l / 2), 2 * round(h / 1.2 ** l / 2)) for l in range(8)]
    assert max(round((wl - 32) / (hl - 32)) for wl, hl in sizes) == 16                # kMaxRoots, on the top level
    assert pc.check_extractor(lib, w, h, nfeatures, stages=True) == len(okps)


def check_extractor_side_refused(lib):
    """widths and heights of 4097: RGBL_ERR_INVALID that names 4096, no handle; 4096 is taken"""
    for w, h in ((SIDE_MAX + 1, 288), (288, SIDE_MAX + 1), (SIDE_MAX + 1, SIDE_MAX + 1)):
        cfg = L.ExtractorCfg(500, 1.2, 4, 20, 7, w, h, 1)
        handle = C.c_void_p(0x5a)
        assert lib.rgbl_extractor_create(C.byref(cfg), 0, C.byref(handle)) == L.ERR_INVALID, (w, h)
        assert b"4096" in lib.rgbl_last_error() and not handle.value
    F.ORBextractor(500, 1.2, 1, 20, 7, SIDE_MAX, 288, lib=lib).close()
    F.ORBextractor(500, 1.2, 1, 20, 7, SIDE_MAX, SIDE_MAX, lib=lib).close()       # (a portrait image has no quad-tree root)


def largest_nfeatures(lib, w, h):
    """the largest nfeatures rgbl_extractor_create takes for one level of w x h, by bisection (no kernel runs), and the message of
    the refusal above it"""
    def accepted(n):
        try:
            F.ORBextractor(n, 1.2, 1, 20, 7, w, h, lib=lib).close()
            return True, ""
        except L.RgblError as e:
            assert e.code == L.ERR_INVALID
            return False, str(e)
    lo, hi = 1000, 1 << 17
    assert accepted(lo)[0] and not accepted(hi)[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if accepted(mid)[0]:
            lo = mid
        else:
            hi = mid
    return lo, accepted(lo + 1)[1]


def check_extractor_node_list_limit(lib, w=2048, h=1024):
    """One level, the largest nfeatures the library takes, uniform noise: list positions up to the top of the 16-bit field"""
    import parity_checks as pc
    nfeatures, refusal = largest_nfeatures(lib, w, h)
    assert "65535" in refusal and nfeatures + 24 <= 65535 < nfeatures + 64, (nfeatures, refusal)
    img = np.random.default_rng(77).integers(0, 256, (h, w), dtype=np.uint8)
    orc = O.Extractor(nfeatures, 1.2, 1, 20, 7)
    okps, odesc, omono = orc(img)
    assert len(okps) >= 60000, len(okps)                                   # (a) and (b): the node list reaches beyond 2^15 entries
    ex = F.ORBextractor(nfeatures, 1.2, 1, 20, 7, w, h, lib=lib)
    kps, desc, mono = ex(img)
    pc.assert_keypoints_equal(kps, okps, "%d features on one level" % nfeatures)
    assert np.array_equal(desc, odesc) and mono == omono
    ex.close()
    return nfeatures


# ---- 10. xcd_grid (csrc/common.h): more than 65535 items per frame take the plain grid (items, 1, frames) -------------------------
_plain_grid = {}


def _plain_grid_reference(w, h, nlevels, scale, nfeatures):
    """two images and the oracle's extraction of each: computed once (a dozen seconds apiece), shared, never modified"""
    from orb_slam3_rgbl_amd import synth
    key = (w, h, nlevels, scale, nfeatures)
    if key not in _plain_grid:
        seq = synth.Sequence(12, w, h, n_frames=2)
        imgs = [seq.frame(0), seq.frame(1)]
        orc = O.Extractor(nfeatures, scale, nlevels, 20, 7)
        _plain_grid[key] = (imgs, [orc(im) for im in imgs])
    return _plain_grid[key]


def check_extractor_plain_grid(lib, batch, xcd_map=True, w=SIDE_MAX, h=SIDE_MAX, nlevels=16, scale=1.1, nfeatures=3000):
    """A 4096 x 4096 image on 16 levels at 1.1 has more than 65535 detection cells.  The schedules launch the FAST cells level range
    by level range, none of which reaches that count; with per-kernel timing on (one stream) ONE launch covers the cells of every
    level: that launch takes the plain grid.  Keypoints and descriptors against the oracle, bit for bit; two distinct images take
    turns in a batch."""
    import os

    import parity_checks as pc
    saved = os.environ.pop("RGBL_XCD_MAP", None)
    if not xcd_map:
        os.environ["RGBL_XCD_MAP"] = "0"
    try:
        ex = F.ORBextractor(nfeatures, scale, nlevels, 20, 7, w, h, max_batch=batch, lib=lib)
    finally:
        os.environ.pop("RGBL_XCD_MAP", None)
        if saved is not None:
            os.environ["RGBL_XCD_MAP"] = saved
    try:
        cells = 0
        for l in range(nlevels):       # csrc/extractor.hip, build_geometry: the detection grid of ORBextractor.cc:789-803
            wl, hl = ex.level_size(l)
            cells += int((wl - 16 - 16) / 35.0) * int((hl - 16 - 16) / 35.0)
        assert cells > 65535, cells
        ex.profile(True)
        imgs, want = _plain_grid_reference(w, h, nlevels, scale, nfeatures)
        for okps, _, _ in want:
            gc.assert_floor(len(okps), nfeatures, "%d x %d on %d levels" % (w, h, nlevels))
            assert len(set(okps["octave"].tolist())) == nlevels                      # every level's cells found corners
        if batch == 1:
            got = [ex(imgs[0])]
        else:
            got = ex.extract_batch(np.stack([imgs[b % 2] for b in range(batch)]))
        launches = {name: n for name, (_, n) in ex.profile_read().items()}
        assert launches["k_fast_cells"] == 1, launches                               # one launch over all the cells
        for b, (kps, desc, mono) in enumerate(got):
            okps, odesc, omono = want[b % 2]
            pc.assert_keypoints_equal(kps, okps, "frame %d of %d" % (b, batch))
            assert np.array_equal(desc, odesc) and mono == omono
        return cells
    finally:
        ex.close()


def check_resize_plain_grid(lib, sizes=(2048, 1028, 16384, 8224)):
    """rgbl_resize to a destination of more than 65535 tiles of 64 x 32: k_resize on the plain grid, against tests/resize_ref.py"""
    import resize_cases as rc
    sw, sh, dw, dh = sizes
    tiles = -(-dw // 64) * -(-dh // 32)
    assert tiles > 65535, tiles
    rc.check_host_case(lib, sizes, 1)
    return tiles
