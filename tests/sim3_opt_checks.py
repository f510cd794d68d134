"""rgbl_optimize_sim3 / _batch / _host - Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381), one workgroup per candidate: the
checks tests/test_sim3_opt_emu.py runs with the kernel under the SIMT emulator and tests/test_sim3_opt_gpu.py on the MI355X.
The yardstick is the HOST build of csrc/sim3opt_math.h in the same library (rgbl_optimize_sim3_host), bit for bit: estimate,
flags, count, counters and diagnostics.  tests/test_sim3_opt_math.py holds that host build to the float64 model of
tests/sim3_opt_model.py.  NaN diagnostics are compared as NaN, not by payload."""
import ctypes as C
import threading

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import sim3_cases as sc

# no edge, both sides of the `< 10` return, one pair per lane on both sides, the global-memory loop (more than 8 x 256)
SIZES = (0, 9, 10, 11, 255, 256, 257, 2048, 2049)
COUNTERS = ("n_correspondences", "n_bad_mps", "n_in_kf2", "n_out_kf2", "n_without_mp", "n_bad")
CASE_KEYS = ("mp1_index", "match_index", "i2", "track_level2", "bad", "world_pos", "Rcw1", "tcw1", "Rcw2", "tcw2", "xy1", "octave1",
             "xy2", "octave2", "n2", "inv_level_sigma2_1", "inv_level_sigma2_2", "K1", "K2", "R", "t", "s", "th2", "fix_scale",
             "all_points")
FILL = 7   # what the cleared flags hold before a call: a byte the call never writes


def sized_case(matched, fix_scale=False, seed=0, **kw):
    """`matched` correspondences exactly: every match has both points, is seen in key frame 2 and lies in front of it"""
    n = max(matched + matched // 3, 4)
    kw.setdefault("outlier_share", 0.1 if matched >= 20 else 0.0)
    return sc.make_sim3_opt_case(n, matched, seed=2000 + 7 * matched + seed, fix_scale=fix_scale, **kw)


def same(got, want, what):
    assert got["result"] == want["result"] and got["rounds"] == want["rounds"], (what, got["result"], want["result"], got["rounds"], want["rounds"])
    for k in COUNTERS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("iterations", "active"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert np.array_equal(got["cleared"], want["cleared"]), (what, "cleared", np.nonzero(got["cleared"] != want["cleared"])[0][:8])
    for k in ("q", "t"):
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (what, k, got[k], want[k])
    assert np.float64(got["s"]).view(np.uint64) == np.float64(want["s"]).view(np.uint64), (what, "s", got["s"], want["s"])
    nan = np.isnan(want["chi2"])
    assert np.array_equal(np.isnan(got["chi2"]), nan), (what, "chi2", got["chi2"], want["chi2"])
    assert np.array_equal(got["chi2"][~nan].view(np.uint64), want["chi2"][~nan].view(np.uint64)), (what, "chi2", got["chi2"], want["chi2"])


def entry_bits_kept(res, case):
    q = F.quat_from_matrix(case["R"])
    return (np.array_equal(res["q"].view(np.uint64), q.view(np.uint64)) and np.array_equal(res["t"], np.asarray(case["t"], np.float64))
            and res["s"] == float(case["s"]))


def check_size(lib, mt, matched, fix_scale):
    """device against host build, bit for bit; returns the host's result dict"""
    case = sized_case(matched, fix_scale)
    want = F.optimize_sim3_host(case, lib, cleared_fill=FILL)
    got = mt.OptimizeSim3(case, cleared_fill=FILL)
    same(got, want, "%d matched, fix_scale %d" % (matched, fix_scale))
    assert want["n_correspondences"] == matched and want["n_in_kf2"] == matched and want["active"][0] == matched
    has_pair = np.asarray(case["match_index"]) >= 0
    assert np.all(want["cleared"][~has_pair] == FILL) and np.all(want["cleared"][has_pair] <= 1), "a flag was written where no pair existed"
    if matched - want["n_bad"] < 10:
        assert want["result"] == 0 and want["rounds"] == 1 and want["iterations"][1] == 0 and entry_bits_kept(want, case)
    else:
        assert want["rounds"] == 2 and want["active"][1] == matched - want["n_bad"] and want["result"] > 0.7 * matched
        assert not entry_bits_kept(want, case)
        if fix_scale:
            assert want["s"] == 1.0
    if matched == 0:
        assert want["iterations"][0] == 0
    return want


def degenerate_case(on_plane=2, behind=3):
    """identity key-frame poses; matches behind key frame 2 (skipped) and exactly on its camera plane (kept: with i2 < 0 the
    normalised obs2 is non-finite and the chi2 NaN); a fifth of the matches are not seen in key frame 2, those on the plane among them"""
    return sc.make_sim3_opt_case(90, 60, seed=17, all_points=True, identity_poses=True, n_behind=behind, n_on_plane=on_plane, out_kf2_share=0.2)


def check_degenerate_depth(lib, mt):
    case = degenerate_case()
    # the points on the plane are among the matches without an index in key frame 2
    feat = np.nonzero((np.asarray(case["match_index"]) >= 0))[0]
    on_plane = [i for i in feat if case["world_pos"][case["match_index"][i], 2] == 0.0]
    assert len(on_plane) == 2 and (case["i2"][on_plane] < 0).all()
    want = F.optimize_sim3_host(case, lib, cleared_fill=FILL)
    assert want["n_correspondences"] == 57 and want["n_out_kf2"] == 12, want
    # the factorisation fails in every iteration and every comparison with the NaN chi2 is false: one trial each, no early stop
    assert np.isnan(want["chi2"][0]) and want["iterations"][0] == 5, want
    same(mt.OptimizeSim3(case, cleared_fill=FILL), want, "z == 0 and z < 0")
    case = degenerate_case(on_plane=0)
    want = F.optimize_sim3_host(case, lib, cleared_fill=FILL)
    assert want["n_correspondences"] == 57 and not np.isnan(want["chi2"]).any() and want["rounds"] == 2, want
    behind = [i for i in feat if case["world_pos"][case["match_index"][i], 2] < 0.0]
    assert len(behind) == 3 and (want["cleared"][behind] == FILL).all()
    same(mt.OptimizeSim3(case, cleared_fill=FILL), want, "z < 0")


def no_edge_cases():
    a = sc.make_sim3_opt_case(40, 30, seed=5, null_mp1_share=1.0)            # every pMP1 null
    b = sc.make_sim3_opt_case(40, 30, seed=6, out_kf2_share=1.0)             # nothing seen in key frame 2, bAllPoints false
    c = sc.make_sim3_opt_case(40, 30, seed=7)
    c["match_index"] = np.full(40, -1, np.int32)                            # no match at all
    d = sc.make_sim3_opt_case(40, 30, seed=8)
    d["bad"] = np.ones_like(d["bad"])                                       # every point bad
    return dict(null_mp1=a, not_in_kf2=b, no_match=c, all_bad=d)


def check_no_edge(lib, mt):
    for name, case in no_edge_cases().items():
        want = F.optimize_sim3_host(case, lib, cleared_fill=FILL)
        assert want["result"] == 0 and want["n_correspondences"] == 0 and not want["iterations"].any() and want["rounds"] == 1, (name, want)
        assert (want["cleared"] == FILL).all() and entry_bits_kept(want, case), name
        assert want["n_without_mp"] == (30 if name == "null_mp1" else 0) and want["n_bad_mps"] == (30 if name == "all_bad" else 0), (name, want)
        same(mt.OptimizeSim3(case, cleared_fill=FILL), want, name)


def batch_problems(B):
    sizes = [0, 40, 9, 300, 10, 13, 257, 11, 64, 0, 31]
    out = []
    for b in range(B):
        m = sizes[b % len(sizes)] if b < len(sizes) else sizes[b % len(sizes)] % 37   # beyond the first eleven, small problems
        out.append(sized_case(m, fix_scale=b % 2 == 1, seed=b, out_kf2_share=0.1 if b % 3 == 2 else 0.0, all_points=b % 6 == 2,
                              null_mp1_share=0.1 if b % 4 == 1 else 0.0))
    return out


def check_batch(lib, mt, B):
    problems = batch_problems(B)
    got = mt.OptimizeSim3Batch(problems, cleared_fill=FILL)
    assert len(got) == B
    for b in range(B):
        same(got[b], mt.OptimizeSim3(problems[b], cleared_fill=FILL), "problem %d of %d" % (b, B))
    return sum(g["result"] for g in got)


def check_resident(lib, mt):
    """host arrays against resident frames + a pool whose slots are not the point indices"""
    case = sc.make_sim3_opt_case(500, 320, seed=23, out_kf2_share=0.1, all_points=True, bad_share=0.05, null_mp1_share=0.05)
    n, n2, npts = len(case["match_index"]), int(case["n2"]), len(case["world_pos"])
    want = mt.OptimizeSim3(case, cleared_fill=FILL)
    same(want, F.optimize_sim3_host(case, lib, cleared_fill=FILL), "host arrays")
    fr1 = F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), case["xy1"], case["octave1"])
    fr2 = F.DeviceFrame(n2, lib=lib).upload(np.zeros((n2, 32), np.uint8), case["xy2"], case["octave2"])
    pool = F.MapPointPool(1000, lib=lib)
    slot = np.random.default_rng(1).permutation(1000)[:npts].astype(np.int32)
    pool.update(slot, world_pos=case["world_pos"])
    res = {k: case[k] for k in CASE_KEYS if k not in ("world_pos", "xy1", "octave1", "xy2", "octave2")}
    host_kf = dict(xy1=case["xy1"], octave1=case["octave1"], xy2=case["xy2"], octave2=case["octave2"])
    same(mt.OptimizeSim3(dict(res, device1=fr1, device2=fr2, pool=pool, slot=slot), cleared_fill=FILL), want, "resident frames and pool")
    same(mt.OptimizeSim3(dict(res, device1=fr1, device2=fr2, world_pos=case["world_pos"]), cleared_fill=FILL), want, "resident frames, host points")
    same(mt.OptimizeSim3(dict(res, pool=pool, slot=slot, **host_kf), cleared_fill=FILL), want, "host frames, pool")
    same(mt.OptimizeSim3(dict(res, device1=fr1, xy2=case["xy2"], octave2=case["octave2"], pool=pool, slot=slot), cleared_fill=FILL), want,
         "key frame 1 resident, key frame 2 host")
    same(mt.OptimizeSim3Batch([dict(res, device1=fr1, device2=fr2, pool=pool, slot=slot), case], cleared_fill=FILL)[1], want, "batch of both forms")
    fr1.close()
    fr2.close()
    pool.close()
    return want["result"]


def _structs(base, case, n):
    keep = []
    I, O = (L.Sim3OptInput * 2)(), (L.Sim3OptOutput * 2)()
    clr = [np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)]
    F.ORBmatcher._sim3_opt_input(base, keep, I[0])
    F.ORBmatcher._sim3_opt_input(case, keep, I[1])
    for b in range(2):
        C.memset(C.byref(O[b]), 0x5a, C.sizeof(L.Sim3OptOutput))
        O[b].cleared = clr[b].ctypes.data
    return keep, I, O, clr


def check_errors(lib, mt):
    """every argument error: RGBL_ERR_INVALID, and estimate, flags, count and diagnostics stay as the caller left them"""
    base = sc.make_sim3_opt_case(60, 40, seed=31, out_kf2_share=0.2, all_points=True)
    n, n2 = len(base["match_index"]), int(base["n2"])
    fr = F.DeviceFrame(n + 5, lib=lib).upload(np.zeros((n + 5, 32), np.uint8), np.zeros((n + 5, 2), np.float32), np.zeros(n + 5, np.int32))
    pool = F.MapPointPool(16, lib=lib)

    def broken(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c

    def without(*keys, **more):
        return dict({k: base[k] for k in CASE_KEYS if k not in keys}, **more)
    matched = np.nonzero(np.asarray(base["match_index"]) >= 0)[0]
    first = int(matched[0])
    in2 = int(next(i for i in matched if base["i2"][i] >= 0))
    out2 = int(next(i for i in matched if base["i2"][i] < 0))
    npts = len(base["bad"])
    bad = {"mp1_index too large": broken("mp1_index", first, npts),
           "match_index below -1": broken("match_index", first, -2),
           "i2 too large": broken("i2", in2, n2),
           "i2 below -1": broken("i2", in2, -2),
           "octave1 too large": broken("octave1", first, 8),
           "octave2 negative": broken("octave2", int(base["i2"][in2]), -1),
           "track level too large": broken("track_level2", out2, 8),
           "pose NaN": broken("Rcw2", (1, 1), np.nan),
           "K inf": broken("K1", 0, np.inf),
           "estimate NaN": broken("t", 2, np.nan),
           "th2 NaN": dict(base, th2=np.float32(np.nan)),
           "scale inf": dict(base, s=float("inf")),
           "frame of another size": without("xy1", "octave1", device1=fr),
           "slot outside the pool": without("world_pos", pool=pool, slot=np.arange(npts, dtype=np.int32)),
           "no levels": dict(base, n_levels2=0),
           "no map side": without("world_pos"),
           "no i2 array": without("i2", n=n),
           "no key points of key frame 2": without("xy2")}
    for what, case in bad.items():
        for batch in (False, True):
            keep, I, O, clr = _structs(base, case, n)
            before = [bytes(O[0]), bytes(O[1])]
            if batch:   # the good problem in front of the bad one: neither is written
                rc = lib.rgbl_optimize_sim3_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))
            else:
                rc = lib.rgbl_optimize_sim3(mt.h, C.byref(I[1]), C.byref(O[1]))
            assert rc == L.ERR_INVALID, (what, batch, rc)
            assert [bytes(O[0]), bytes(O[1])] == before and (clr[0] == 9).all() and (clr[1] == 9).all(), (what, batch)
            if what not in ("frame of another size", "slot outside the pool") and not batch:
                assert lib.rgbl_optimize_sim3_host(C.byref(I[1]), C.byref(O[1])) == L.ERR_INVALID, what
                assert bytes(O[1]) == before[1] and (clr[1] == 9).all(), what
    keep, I, O, clr = _structs(base, base, n)
    assert lib.rgbl_optimize_sim3(mt.h, None, None) == L.ERR_INVALID
    assert lib.rgbl_optimize_sim3_host(C.byref(I[0]), None) == L.ERR_INVALID
    assert lib.rgbl_optimize_sim3_batch(mt.h, -1, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == L.ERR_INVALID
    # a level that is out of range on a match that gets no edge is not an error: the reference never reads it
    skipped = broken("track_level2", in2, 99)
    same(mt.OptimizeSim3(skipped), F.optimize_sim3_host(base, lib), "an unused level")
    # the host build refuses resident inputs
    keep = []
    I0 = F.ORBmatcher._sim3_opt_input(without("world_pos", pool=pool, slot=np.zeros(npts, np.int32)), keep)
    O0 = L.Sim3OptOutput()
    assert lib.rgbl_optimize_sim3_host(C.byref(I0), C.byref(O0)) == L.ERR_INVALID
    fr.close()
    pool.close()
    same(mt.OptimizeSim3(base), F.optimize_sim3_host(base, lib), "after the refused calls")


# ---- the limits, from both sides ------------------------------------------------------------------------------------------
N_MAX = 65535


def limit_case(matched=1200, seed=3):
    """N_MAX features in both key frames; the last feature of key frame 1 carries a pair whose match is the last feature of
    key frame 2, and a feature with bit 15 set carries one too"""
    case = sc.make_sim3_opt_case(N_MAX, matched, seed=seed)
    mt_ = case["match_index"]
    last = N_MAX - 1
    if mt_[last] < 0:
        i = int(np.nonzero(mt_ >= 0)[0][matched // 2])
        for k in ("mp1_index", "match_index", "i2", "track_level2", "xy1", "octave1", "planted_outlier"):
            case[k][[i, last]] = case[k][[last, i]]
    # key frame 2 grows to N_MAX features; the last pair's observation moves to its last feature
    n2 = int(case["n2"])
    xy2, oct2 = np.zeros((N_MAX, 2), np.float32), np.zeros(N_MAX, np.int32)
    xy2[:n2], oct2[:n2] = case["xy2"], case["octave2"]
    j = int(case["i2"][last])
    xy2[last], oct2[last] = xy2[j], oct2[j]
    case["i2"][last] = last
    case.update(xy2=xy2, octave2=oct2, n2=N_MAX)
    assert mt_[last] >= 0 and (mt_[32768:last] >= 0).any() and int((mt_ >= 0).sum()) == matched
    return case


def check_limit(lib, mt):
    case = limit_case()
    want = F.optimize_sim3_host(case, lib, cleared_fill=FILL)
    assert want["rounds"] == 2 and want["n_correspondences"] == 1200 and want["result"] > 900, want
    assert want["cleared"][N_MAX - 1] != FILL
    same(mt.OptimizeSim3(case, cleared_fill=FILL), want, "%d features" % N_MAX)
    # the other value of the last pair's flag: its observation in key frame 2 moved 40 px away
    far = dict(case, xy2=case["xy2"].copy())
    far["xy2"][N_MAX - 1] += np.float32(40.0 if not want["cleared"][N_MAX - 1] else -40.0)
    want2 = F.optimize_sim3_host(far, lib, cleared_fill=FILL)
    assert want2["cleared"][N_MAX - 1] == 1
    same(mt.OptimizeSim3(far, cleared_fill=FILL), want2, "%d features, the last pair dropped" % N_MAX)
    return want["result"]


def check_levels_limit(lib, mt):
    """16 pyramid levels are accepted - with a pair on level 15 of either key frame -, 17 refused"""
    case = sc.make_sim3_opt_case(120, 80, seed=9, n_levels=16, scale_factor=1.1)
    matched = np.nonzero(np.asarray(case["match_index"]) >= 0)[0]
    case["octave1"][matched[0]] = 15
    case["octave2"][case["i2"][matched[1]]] = 15
    want = F.optimize_sim3_host(case, lib)
    assert want["rounds"] == 2 and want["n_correspondences"] == 80
    same(mt.OptimizeSim3(case), want, "16 levels")
    for side in ("1", "2"):
        more = dict(case, **{"inv_level_sigma2_" + side: np.append(case["inv_level_sigma2_" + side], np.float32(0.2))})
        keep, I, O, clr = _structs(case, more, 120)
        before = bytes(O[1])
        for rc in (lib.rgbl_optimize_sim3(mt.h, C.byref(I[1]), C.byref(O[1])), lib.rgbl_optimize_sim3_host(C.byref(I[1]), C.byref(O[1])),
                   lib.rgbl_optimize_sim3_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))):
            assert rc == L.ERR_INVALID and b"16" in lib.rgbl_last_error(), (side, rc, lib.rgbl_last_error())
        assert bytes(O[1]) == before and (clr[0] == 9).all() and (clr[1] == 9).all()


def check_limit_refused(lib, mt):
    """n or n2 = 65536 (refused before an array is read) and 32768 problems: RGBL_ERR_INVALID that names the limit, nothing written"""
    base = sc.make_sim3_opt_case(60, 40, seed=31)
    for field in ("n", "n2"):
        for entry in ("single", "batch", "host"):
            keep, I, O, clr = _structs(base, base, 60)
            setattr(I[1], field, N_MAX + 1)
            before = [bytes(O[0]), bytes(O[1])]
            rc = {"single": lambda: lib.rgbl_optimize_sim3(mt.h, C.byref(I[1]), C.byref(O[1])),
                  "batch": lambda: lib.rgbl_optimize_sim3_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)),
                  "host": lambda: lib.rgbl_optimize_sim3_host(C.byref(I[1]), C.byref(O[1]))}[entry]()
            assert rc == L.ERR_INVALID and b"65535" in lib.rgbl_last_error(), (field, entry, rc, lib.rgbl_last_error())
            assert [bytes(O[0]), bytes(O[1])] == before and (clr[0] == 9).all() and (clr[1] == 9).all(), (field, entry)
    keep, I, O, clr = _structs(base, base, 60)
    before = [bytes(O[0]), bytes(O[1])]
    rc = lib.rgbl_optimize_sim3_batch(mt.h, 32768, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))   # refused before problem 2 is read
    assert rc == L.ERR_INVALID and b"32767" in lib.rgbl_last_error(), (rc, lib.rgbl_last_error())
    assert [bytes(O[0]), bytes(O[1])] == before and (clr[0] == 9).all()
    same(mt.OptimizeSim3(base), F.optimize_sim3_host(base, lib), "after the refused calls")


def check_threads(lib, rounds=4):
    """the call next to other matcher calls from other threads, every thread on a handle of its own"""
    case = sc.make_sim3_opt_case(600, 400, seed=41)
    want = F.optimize_sim3_host(case, lib)
    kfa, kfb, K, R, t, ep, sf, s2 = cases.make_triangulation_case(400, 11, 30)
    m0 = F.ORBmatcher(0.6, False, lib=lib)
    Fm = m0.fundamental(K, K, R, t)
    want_tri = m0.SearchForTriangulation(kfa, kfb, Fm, ep, sf, s2)[2].copy()
    errors = []

    def guarded(body):
        def f():
            try:
                body()
            except Exception as ex:   # noqa: BLE001
                errors.append(ex)
        return f

    def optimise():
        m = F.ORBmatcher(0.6, False, lib=lib)
        for r in range(rounds):
            same(m.OptimizeSim3(case), want, "round %d next to searches" % r)
        m.close()

    def search():
        m = F.ORBmatcher(0.6, False, lib=lib)
        for r in range(rounds):
            assert np.array_equal(m.SearchForTriangulation(kfa, kfb, Fm, ep, sf, s2)[2], want_tri)
        m.close()
    threads = [threading.Thread(target=guarded(f)) for f in (optimise, search, optimise, search)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    m0.close()
    assert not errors, errors


def check_math_device(lib):
    """the header's exp and the fp64 quotient and square root: device against host, bit for bit, on a sweep"""
    lib.rgbl_test_so_exp.restype, lib.rgbl_test_so_exp.argtypes = C.c_double, [C.c_double]
    lib.rgbl_test_so_exp_device.restype, lib.rgbl_test_so_exp_device.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    lib.rgbl_test_po_math.restype, lib.rgbl_test_po_math.argtypes = C.c_double, [C.c_int, C.c_double, C.c_double]
    lib.rgbl_test_po_math_device.restype = C.c_int
    lib.rgbl_test_po_math_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    rng = np.random.default_rng(5)
    special = np.array([0.0, -0.0, 1e-9, -1e-9, 1e-5, 0.5 * np.log(2), 1.5 * np.log(2), 2.0 ** -28, 2.0 ** -29, 709.78, 709.79, 710.0,
                        -745.13, -745.14, -746.0, -708.4, -1000.0, 1e300, np.inf, -np.inf, np.nan, 5e-324])
    x = np.concatenate([rng.uniform(-1, 1, 1 << 14), rng.uniform(-1e-4, 1e-4, 1 << 13), rng.uniform(-746, 710, 1 << 14), special])
    got = np.zeros(len(x))
    assert lib.rgbl_test_so_exp_device(x.ctypes.data, got.ctypes.data, len(x)) == 0
    want = np.array([lib.rgbl_test_so_exp(float(a)) for a in x])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = got[~nan].view(np.uint64) != want[~nan].view(np.uint64)
    assert not bad.any(), ("exp", x[~nan][bad][:8])
    y = np.concatenate([rng.uniform(-1e3, 1e3, len(x) - 6) * 10.0 ** rng.integers(-300, 300, len(x) - 6), np.array([0.0, -0.0, np.inf, np.nan, 5e-324, 1e308])])
    z = np.abs(x) * 10.0 ** rng.integers(-150, 150, len(x))
    for op, name, a in ((2, "quotient", x), (3, "sqrt", z)):
        assert lib.rgbl_test_po_math_device(op, a.ctypes.data, y.ctypes.data, got.ctypes.data, len(a)) == 0
        want = np.array([lib.rgbl_test_po_math(op, float(p), float(q)) for p, q in zip(a, y)])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), name
        bad = got[~nan].view(np.uint64) != want[~nan].view(np.uint64)
        assert not bad.any(), (name, a[~nan][bad][:8], y[~nan][bad][:8])
    return len(x)
