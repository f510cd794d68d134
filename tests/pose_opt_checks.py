"""rgbl_pose_optimization / _batch / _host - Optimizer::PoseOptimization (src/Optimizer.cc:814-1114), one workgroup per frame:
the checks tests/test_pose_opt_emu.py runs with the kernel under the SIMT emulator and tests/test_pose_opt_gpu.py on the
MI355X.  The yardstick is the HOST build of csrc/poseopt_math.h in the same library (rgbl_pose_optimization_host), bit for bit:
pose, flags, count and diagnostics.  tests/test_pose_opt_math.py holds that host build to the float64 model of
tests/pose_opt_model.py.  NaN diagnostics are compared as NaN, not by payload (the sign of a generated NaN is the machine's)."""
import ctypes as C
import threading

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F

# the return-0 path, the `< 10` break, one edge per lane on both sides, the global-memory loop (more than 8 x 256)
SIZES = (0, 2, 3, 9, 10, 255, 256, 257, 2049)
KINDS = {"mono": 1.0, "stereo": 0.0, "mixed": 0.3}
FRAME_KEYS = ("mp_index", "world_pos", "xy", "octave", "uright", "q", "t", "K", "bf", "inv_level_sigma2", "n_levels")


def sized_case(matched, kind, seed=0):
    n = max(matched + matched // 3, 4)
    return cases.make_pose_opt_case(n, matched, seed=1000 + 7 * matched + seed, mono_share=KINDS[kind])


def same(got, want, what):
    for k in ("q", "t"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k, got[k], want[k])
    assert np.array_equal(got["outlier"], want["outlier"]), (what, "outlier", np.nonzero(got["outlier"] != want["outlier"])[0][:8])
    assert got["result"] == want["result"] and got["rounds"] == want["rounds"], (what, got["result"], want["result"])
    for k in ("iterations", "active"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("q64", "t64"):
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (what, k, got[k], want[k])
    nan = np.isnan(want["chi2"])
    assert np.array_equal(np.isnan(got["chi2"]), nan), (what, "chi2", got["chi2"], want["chi2"])
    assert np.array_equal(got["chi2"][~nan].view(np.uint64), want["chi2"][~nan].view(np.uint64)), (what, "chi2", got["chi2"], want["chi2"])


def check_size(lib, mt, matched, kind):
    """device against host build, bit for bit; returns the host's result dict"""
    case = sized_case(matched, kind)
    want = F.pose_optimization_host(case, lib, outlier_fill=7)
    got = mt.PoseOptimization(case, outlier_fill=7)
    same(got, want, "%d matched, %s" % (matched, kind))
    assert np.all(want["outlier"][case["mp_index"] < 0] == 7), "a flag was written where there is no map point"
    if matched < 3:
        assert want["result"] == 0 and want["rounds"] == 0 and not want["outlier"][case["mp_index"] >= 0].any()
        assert np.array_equal(want["q"].view(np.uint32), case["q"].view(np.uint32)) and np.array_equal(want["t"], case["t"])
    else:
        assert want["rounds"] == (1 if matched < 10 else 4), want["rounds"]
        assert want["active"][0] == matched
    return want


def all_outliers_case():
    """observations that have nothing to do with the points: every edge is an outlier after round 0, the later rounds have an
    empty active set and run no iteration"""
    case = cases.make_pose_opt_case(80, 60, seed=5, mono_share=0.3)
    rng = np.random.default_rng(9)
    case["xy"] = (case["xy"] + rng.choice([-1.0, 1.0], case["xy"].shape) * rng.uniform(150, 400, case["xy"].shape)).astype(np.float32)
    return case


def check_all_outliers(lib, mt):
    case = all_outliers_case()
    want = F.pose_optimization_host(case, lib)
    assert want["result"] == 0 and want["active"][0] == 60 and not want["active"][1:].any() and not want["iterations"][1:].any(), want
    assert want["outlier"][case["mp_index"] >= 0].all()
    same(mt.PoseOptimization(case), want, "all outliers")


def degenerate_depth_case(stereo):
    """the identity pose, exactly: one point with z == 0 (a non-finite error: the factorisation fails in every trial) and one
    behind the camera"""
    case = cases.make_pose_opt_case(40, 30, seed=17, mono_share=0.0 if stereo else 1.0, rot_noise=0.0, trans_noise=0.0)
    R = cases._rot(case["q_true"])
    Xc = case["world_pos"].astype(np.float64) @ R.T + case["t_true"].astype(np.float64)
    case["world_pos"] = Xc.astype(np.float32)
    case["q"], case["t"] = np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32)
    case["world_pos"][3, 2] = 0.0
    case["world_pos"][11, 2] = -5.0
    return case


def check_degenerate_depth(lib, mt):
    for stereo in (False, True):
        case = degenerate_depth_case(stereo)
        want = F.pose_optimization_host(case, lib)
        assert want["rounds"] == 4 and np.isnan(want["chi2"]).any(), want   # the non-finite path was taken, and it ended
        assert (want["iterations"] == 10).all(), want                      # every comparison with NaN is false: no early stop
        same(mt.PoseOptimization(case), want, "z == 0 and z < 0, stereo %d" % stereo)
        case["world_pos"][3, 2] = 12.0                                     # only the point behind the camera
        want = F.pose_optimization_host(case, lib)
        assert not np.isnan(want["chi2"]).any()
        same(mt.PoseOptimization(case), want, "z < 0, stereo %d" % stereo)


def batch_frames(B):
    sizes = [0, 40, 2, 300, 9, 13, 257, 3, 64, 0, 31]
    kinds = list(KINDS)
    # beyond the first eleven, small problems: more workgroups than CUs is what B = 300 is about
    return [sized_case(sizes[b % len(sizes)] if b < len(sizes) else sizes[b % len(sizes)] % 37, kinds[b % 3], seed=b) for b in range(B)]


def check_batch(lib, mt, B):
    frames = batch_frames(B)
    got = mt.PoseOptimizationBatch(frames, outlier_fill=5)
    assert len(got) == B
    for b in range(B):
        same(got[b], mt.PoseOptimization(frames[b], outlier_fill=5), "problem %d of %d" % (b, B))
    return sum(g["result"] for g in got)


def check_resident(lib, mt):
    """host arrays against a resident frame + a pool whose slots are not the point indices"""
    case = cases.make_pose_opt_case(500, 320, seed=23)
    n, npts = len(case["mp_index"]), len(case["world_pos"])
    want = mt.PoseOptimization(case)
    fr = F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), case["xy"], case["octave"], case["uright"])
    pool = F.MapPointPool(1000, lib=lib)
    slot = np.random.default_rng(1).permutation(1000)[:npts].astype(np.int32)
    pool.update(slot, world_pos=case["world_pos"])
    res = {k: case[k] for k in ("mp_index", "q", "t", "K", "bf", "inv_level_sigma2", "n_levels")}
    same(mt.PoseOptimization(dict(res, device=fr, pool=pool, slot=slot)), want, "resident frame and pool")
    same(mt.PoseOptimization(dict(res, device=fr, world_pos=case["world_pos"])), want, "resident frame, host points")
    same(mt.PoseOptimization(dict(res, xy=case["xy"], octave=case["octave"], uright=case["uright"], pool=pool, slot=slot)), want, "host frame, pool")
    same(mt.PoseOptimizationBatch([dict(res, device=fr, pool=pool, slot=slot), case])[1], want, "batch of both forms")
    fr.close()
    pool.close()
    return want["result"]


def check_errors(lib, mt):
    """every argument error: RGBL_ERR_INVALID, and pose, flags, count and diagnostics stay as the caller left them"""
    base = cases.make_pose_opt_case(60, 40, seed=31)
    n = len(base["mp_index"])
    fr = F.DeviceFrame(n + 5, lib=lib).upload(np.zeros((n + 5, 32), np.uint8), np.zeros((n + 5, 2), np.float32), np.zeros(n + 5, np.int32))
    pool = F.MapPointPool(16, lib=lib)

    def broken(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c
    first = int(np.nonzero(base["mp_index"] >= 0)[0][0])
    bad = {"mp_index too large": broken("mp_index", first, len(base["world_pos"])),
           "mp_index below -1": broken("mp_index", first, -2),
           "octave too large": broken("octave", first, 8),
           "octave negative": broken("octave", first, -1),
           "pose NaN": broken("q", 1, np.nan),
           "translation inf": broken("t", 2, np.inf),
           "frame of another size": dict({k: base[k] for k in FRAME_KEYS if k not in ("xy", "octave", "uright")}, device=fr),
           "slot outside the pool": dict({k: base[k] for k in FRAME_KEYS if k != "world_pos"}, pool=pool,
                                         slot=np.arange(len(base["world_pos"]), dtype=np.int32)),
           "no levels": dict(base, n_levels=0),
           "no map side": dict({k: base[k] for k in FRAME_KEYS if k != "world_pos"}, n_points=len(base["world_pos"]))}
    for what, case in bad.items():
        for batch in (False, True):
            keep = []
            I = (L.PoseOptInput * 2)()
            O = (L.PoseOptOutput * 2)()
            outl = [np.full(n, 9, np.uint8), np.full(n, 9, np.uint8)]
            F.ORBmatcher._pose_opt_input(base, keep, I[0])
            F.ORBmatcher._pose_opt_input(case, keep, I[1])
            for b in range(2):
                C.memset(C.byref(O[b]), 0x5a, C.sizeof(L.PoseOptOutput))
                O[b].outlier = outl[b].ctypes.data
            before = [bytes(O[0]), bytes(O[1])]
            if batch:   # the good problem in front of the bad one: neither is written
                rc = lib.rgbl_pose_optimization_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))
            else:
                rc = lib.rgbl_pose_optimization(mt.h, C.byref(I[1]), C.byref(O[1]))
            assert rc == L.ERR_INVALID, (what, batch, rc)
            assert [bytes(O[0]), bytes(O[1])] == before and (outl[0] == 9).all() and (outl[1] == 9).all(), (what, batch)
            if what not in ("frame of another size", "slot outside the pool") and not batch:
                C.memset(C.byref(O[1]), 0x5a, C.sizeof(L.PoseOptOutput))
                O[1].outlier = outl[1].ctypes.data
                assert lib.rgbl_pose_optimization_host(C.byref(I[1]), C.byref(O[1])) == L.ERR_INVALID, what
                assert bytes(O[1]) == before[1] and (outl[1] == 9).all(), what
    assert lib.rgbl_pose_optimization(mt.h, None, None) == L.ERR_INVALID
    assert lib.rgbl_pose_optimization_host(C.byref(I[0]), None) == L.ERR_INVALID
    # the host build refuses resident inputs
    keep = []
    I0 = F.ORBmatcher._pose_opt_input(dict({k: base[k] for k in FRAME_KEYS if k != "world_pos"}, pool=pool,
                                           slot=np.zeros(len(base["world_pos"]), np.int32)), keep)
    O0 = L.PoseOptOutput()
    assert lib.rgbl_pose_optimization_host(C.byref(I0), C.byref(O0)) == L.ERR_INVALID
    fr.close()
    pool.close()
    same(mt.PoseOptimization(base), F.pose_optimization_host(base, lib), "after the refused calls")


# ---- n <= 65535: an edge names its feature in 16 bits ------------------------------------------------------------------------
N_MAX = 65535
PER_FEATURE = ("mp_index", "xy", "octave", "uright", "planted_outlier")


def limit_case(matched=30000, seed=3):
    """N_MAX features, `matched` with a map point; the last feature (65534) carries an edge, and so does one with bit 15 set"""
    case = cases.make_pose_opt_case(N_MAX, matched, seed=seed)
    mp = case["mp_index"]
    if mp[N_MAX - 1] < 0:
        i = int(np.nonzero(mp >= 0)[0][matched // 2])
        for k in PER_FEATURE:
            case[k][[i, N_MAX - 1]] = case[k][[N_MAX - 1, i]]
    assert mp[N_MAX - 1] >= 0 and (mp[32768:N_MAX - 1] >= 0).any() and int((mp >= 0).sum()) == matched
    return case


def check_limit(lib, mt):
    case = limit_case()
    want = F.pose_optimization_host(case, lib, outlier_fill=7)
    assert want["rounds"] == 4 and want["active"][0] == 30000 and want["result"] > 20000, want
    assert want["outlier"][N_MAX - 1] != 7 and (want["outlier"][case["mp_index"] < 0] == 7).all()
    same(mt.PoseOptimization(case, outlier_fill=7), want, "%d features" % N_MAX)
    # the other value of the last edge's flag: its observation moved 40 px away
    far = dict(case, xy=case["xy"].copy())
    far["xy"][N_MAX - 1] += np.float32(40.0 if not want["outlier"][N_MAX - 1] else 0.0)
    want2 = F.pose_optimization_host(far, lib, outlier_fill=7)
    assert want2["outlier"][N_MAX - 1] == 1
    same(mt.PoseOptimization(far, outlier_fill=7), want2, "%d features, the last edge an outlier" % N_MAX)
    return want["result"]


def check_limit_refused(lib, mt):
    """n = 65536 (refused before an array is read): RGBL_ERR_INVALID that names 65535, nothing written, by all three entry points"""
    base = cases.make_pose_opt_case(60, 40, seed=31)
    for entry in ("single", "batch", "host"):
        keep = []
        I, O = (L.PoseOptInput * 2)(), (L.PoseOptOutput * 2)()
        outl = [np.full(60, 9, np.uint8), np.full(60, 9, np.uint8)]
        for b in range(2):
            F.ORBmatcher._pose_opt_input(base, keep, I[b])
            C.memset(C.byref(O[b]), 0x5a, C.sizeof(L.PoseOptOutput))
            O[b].outlier = outl[b].ctypes.data
        I[1].n = N_MAX + 1
        before = [bytes(O[0]), bytes(O[1])]
        rc = {"single": lambda: lib.rgbl_pose_optimization(mt.h, C.byref(I[1]), C.byref(O[1])),
              "batch": lambda: lib.rgbl_pose_optimization_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)),
              "host": lambda: lib.rgbl_pose_optimization_host(C.byref(I[1]), C.byref(O[1]))}[entry]()
        assert rc == L.ERR_INVALID and b"65535" in lib.rgbl_last_error(), (entry, rc, lib.rgbl_last_error())
        assert [bytes(O[0]), bytes(O[1])] == before and (outl[0] == 9).all() and (outl[1] == 9).all(), entry
    same(mt.PoseOptimization(base), F.pose_optimization_host(base, lib), "after the refused calls")


def check_threads(lib, rounds=4):
    """the call next to other matcher calls from other threads, every thread on a handle of its own"""
    case = cases.make_pose_opt_case(600, 400, seed=41)
    want = F.pose_optimization_host(case, lib)
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

    def pose():
        m = F.ORBmatcher(0.6, False, lib=lib)
        for r in range(rounds):
            same(m.PoseOptimization(case), want, "round %d next to searches" % r)
        m.close()

    def search():
        m = F.ORBmatcher(0.6, False, lib=lib)
        for r in range(rounds):
            assert np.array_equal(m.SearchForTriangulation(kfa, kfb, Fm, ep, sf, s2)[2], want_tri)
        m.close()
    threads = [threading.Thread(target=guarded(f)) for f in (pose, search, pose, search)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    m0.close()
    assert not errors, errors


def check_math_device(lib):
    """the header's sin / cos and the fp64 quotient and square root: device against host, bit for bit, on a sweep"""
    lib.rgbl_test_po_math.restype, lib.rgbl_test_po_math.argtypes = C.c_double, [C.c_int, C.c_double, C.c_double]
    lib.rgbl_test_po_math_device.restype = C.c_int
    lib.rgbl_test_po_math_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    rng = np.random.default_rng(3)
    lo, hi = np.array([1e-9, 1e6], np.float64).view(np.uint64)
    x = np.concatenate([np.linspace(int(lo), int(hi), 1 << 15).astype(np.uint64).view(np.float64), rng.uniform(-8, 8, 1 << 14),
                        np.array([0.0, -0.0, 1e-5, np.pi / 4, np.pi / 2, np.pi, 1048576.0, 1048577.0, 1e300, np.inf, -np.inf, np.nan, 5e-324])])
    y = np.concatenate([rng.uniform(-1e3, 1e3, len(x) - 6) * 10.0 ** rng.integers(-300, 300, len(x) - 6), np.array([0.0, -0.0, np.inf, np.nan, 5e-324, 1e308])])
    got = np.zeros(len(x))
    for op, name in enumerate(("sin", "cos", "quotient", "sqrt")):
        assert lib.rgbl_test_po_math_device(op, x.ctypes.data, y.ctypes.data, got.ctypes.data, len(x)) == 0
        want = np.array([lib.rgbl_test_po_math(op, float(a), float(b)) for a, b in zip(x, y)])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), name
        bad = got[~nan].view(np.uint64) != want[~nan].view(np.uint64)
        assert not bad.any(), (name, x[~nan][bad][:8], y[~nan][bad][:8])
    return len(x)
