"""rgbl_sim3_ransac / _batch / _host - Sim3Solver (src/Sim3Solver.cc), every hypothesis of a call at once: the checks
tests/test_sim3_emu.py runs with the kernels under the SIMT emulator and tests/test_sim3_gpu.py on the MI355X.  The yardstick is
the HOST build of csrc/sim3_math.h in the same library (rgbl_sim3_ransac_host), bit for bit: T12, R12, t12, s12, counts, T12_all,
selected, converged, iterations_run and inlier.  tests/test_sim3_math.py holds that host build to the float64 model of
tests/sim3_model.py.  NaN entries are compared as NaN, not by payload (the sign of a generated NaN is the machine's)."""
import ctypes as C
import threading

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import sim3_cases as sc

# chunk edges (63, 64, 65), several chunks per lane (257), the LDS / global switch (1024 points fit: 1025 read global memory)
NS = (3, 20, 63, 64, 65, 257, 1025)
# the workgroup edge at four hypotheses, the selection scan's edge at 64 (300 = 4 chunks and a part)
NHYPS = (1, 3, 4, 5, 20, 300)
FILL = 7


def same_bits(a, b, what):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), (what, "NaN pattern")
    assert np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)), (what, a[~nan][:8], b[~nan][:8])


def same(got, want, what):
    for k in ("selected", "converged", "n_inliers", "iterations_run"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("T12", "R12", "t12", "s12", "T12_all"):
        if want[k] is not None:
            same_bits(got[k], want[k], (what, k))
    if want["counts"] is not None:
        assert np.array_equal(got["counts"], want["counts"]), (what, "counts", np.nonzero(got["counts"] != want["counts"])[0][:8])
    assert np.array_equal(got["inlier"], want["inlier"]), (what, "inlier", np.nonzero(got["inlier"] != want["inlier"])[0][:8])


def sized_case(n, n_hyp, fix_scale, seed=0, **kw):
    kw.setdefault("min_inliers", min(20, max(n // 3, 0)))
    return sc.make_sim3_case(n, n_hyp, seed=100 + 13 * n + n_hyp + seed, fix_scale=fix_scale, **kw)


def check_size(lib, mt, n, n_hyp, fix_scale):
    """device against host build, bit for bit; returns the host's result dict"""
    case = sized_case(n, n_hyp, fix_scale)
    pr = sc.problem(case)
    want = F.sim3_ransac_host(pr, lib, fill=FILL)
    got = mt.Sim3Ransac(pr, fill=FILL)
    same(got, want, "n %d, n_hyp %d, fix_scale %d" % (n, n_hyp, fix_scale))
    assert (want["counts"] >= 0).all() and (want["counts"] <= n).all()
    if want["selected"] >= 0:
        assert want["n_inliers"] == want["counts"][want["selected"]] == int(want["inlier"].sum())
        same_bits(want["T12"], want["T12_all"][want["selected"]], "the selected T12 is its row of T12_all")
        if fix_scale:
            assert want["s12"] == 1.0
    return want


def check_pool(lib, mt):
    """the pool form (slots + key-frame poses, Rcw Xw + tcw on the device) against host arrays"""
    out = 0
    for n in (65, 1025):
        case = sized_case(n, 20, False, seed=3)
        want = mt.Sim3Ransac(sc.problem(case))
        pool = F.MapPointPool(4096, lib=lib)
        perm = np.random.default_rng(n).permutation(4096).astype(np.int32)
        slot1, slot2 = perm[:n], perm[n:2 * n]
        pool.update(np.concatenate([slot1, slot2]), world_pos=np.concatenate([case["Xw1"], case["Xw2"]]))
        same(mt.Sim3Ransac(sc.pool_problem(case, pool, slot1, slot2)), want, "pool form, n %d" % n)
        both = mt.Sim3RansacBatch([sc.pool_problem(case, pool, slot1, slot2), sc.problem(case)])
        same(both[0], want, "batch of both forms, pool")
        same(both[1], want, "batch of both forms, arrays")
        pool.close()
        out += want["n_inliers"]
    return out


def degenerate_case():
    """hypothesis 0: three coincident points; 1: three collinear points; 2: a sample point with z == 0; 3: a triple of planted inliers.
    Correspondence 9 has z == 0 on side 2 (projects to +-inf) and 10 has x = y = z = 0 on side 1 (0 / 0)."""
    case = sized_case(40, 4, False, seed=9)
    x1, x2 = case["x1c"].copy(), case["x2c"].copy()
    x1[1], x2[1] = x1[0], x2[0]
    x1[2], x2[2] = x1[0], x2[0]
    d = np.array([0.5, 0.25, 1.0], np.float32)
    x1[4], x1[5] = x1[3] + d, x1[3] + np.float32(2) * d
    x2[4], x2[5] = x2[3] + d, x2[3] + np.float32(2) * d
    x1[6, 2] = 0.0
    x2[9, 2] = 0.0
    x1[10] = 0.0
    good = [int(i) for i in np.nonzero(case["planted_outlier"] == 0)[0] if i > 10][:3]
    samples = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], good], np.int32)
    return sc.problem(case, x1c=x1, x2c=x2, samples=samples, min_inliers=3)


def check_degenerate(lib, mt):
    pr = degenerate_case()
    want = F.sim3_ransac_host(pr, lib, fill=FILL)
    # coincident points: M = 0, every eigenvalue equal, the first wins: (1, 0, 0, 0), vec.norm() == 0, NaN, no inlier
    assert np.isnan(want["T12_all"][0][:12]).all() and want["counts"][0] == 0, want["T12_all"][0]
    assert want["counts"][3] > 3
    same(mt.Sim3Ransac(pr, fill=FILL), want, "degenerate samples")
    assert not want["inlier"][9] and not want["inlier"][10]
    # every hypothesis NaN: counts all 0, and 0 >= best_inliers = 0 selects the last one - a NaN transformation, as in the reference
    pr2 = dict(pr, samples=np.array([[0, 1, 2], [2, 1, 0]], np.int32), n_hyp=2)
    want = F.sim3_ransac_host(pr2, lib, fill=FILL)
    assert want["selected"] == 1 and want["n_inliers"] == 0 and np.isnan(want["T12"][:3]).all()
    same(mt.Sim3Ransac(pr2, fill=FILL), want, "NaN hypotheses only")


def check_selection(lib, mt):
    """the scan: ties (the later hypothesis wins), a stop at the first c > min_inliers with larger counts behind it, and a
    best_inliers carried in above every count"""
    case = sized_case(257, 300, False, seed=5, outlier_share=0.5)
    pr = sc.problem(case)
    base = F.sim3_ransac_host(pr, lib)
    c = base["counts"]
    top = int(c.max())
    # 1. runs through (min_inliers = n): the LAST hypothesis that reaches the running maximum is held
    pr1 = dict(pr, min_inliers=257)
    w1 = F.sim3_ransac_host(pr1, lib, fill=FILL)
    assert w1["converged"] == 0 and w1["iterations_run"] == 300 and w1["selected"] == int(np.nonzero(c == top)[0][-1])
    same(mt.Sim3Ransac(pr1, fill=FILL), w1, "runs through")
    # 2. a tie made on purpose: the same triple twice (in another order: the same set, maybe other bits) plus an exact copy
    s = case["samples"].copy()
    best = int(np.argmax(c))
    s[-1] = s[best]
    pr2 = dict(pr, samples=s, min_inliers=257)
    w2 = F.sim3_ransac_host(pr2, lib, fill=FILL)
    assert w2["counts"][-1] == top and w2["selected"] == 299
    same(mt.Sim3Ransac(pr2, fill=FILL), w2, "tie: the later hypothesis wins")
    # 3. stops at the first count above a threshold that later hypotheses exceed
    order = np.sort(np.unique(c))
    thr = int(order[len(order) // 2])
    first = int(np.nonzero(c > thr)[0][0])
    assert (c[first + 1:] > c[first]).any(), "the case has no larger count behind the stop"
    pr3 = dict(pr, min_inliers=thr)
    w3 = F.sim3_ransac_host(pr3, lib, fill=FILL)
    assert w3["converged"] == 1 and w3["selected"] == first and w3["iterations_run"] == first + 1
    same(mt.Sim3Ransac(pr3, fill=FILL), w3, "stop at the first c > min_inliers")
    # 4. the stop lies in a later chunk of 64, with updates in the chunks before it
    late = np.nonzero(c > thr)[0]
    late = late[late >= 130]
    assert len(late), "the case has no count above the threshold behind hypothesis 130"
    s4 = case["samples"].copy()
    keep = np.nonzero(c <= thr)[0]
    s4[:int(late[0])] = s4[keep[np.arange(int(late[0])) % len(keep)]]
    pr4 = dict(pr, samples=s4, min_inliers=thr)
    w4 = F.sim3_ransac_host(pr4, lib, fill=FILL)
    assert w4["converged"] == 1 and w4["selected"] == int(late[0]) >= 130
    same(mt.Sim3Ransac(pr4, fill=FILL), w4, "stop in a later chunk")
    # 5. best_inliers above every count: nothing is selected, T12 and the flags stay
    pr5 = dict(pr, best_inliers=top + 1, min_inliers=257)
    w5 = F.sim3_ransac_host(pr5, lib, fill=FILL)
    assert w5["selected"] == -1 and w5["converged"] == 0 and w5["iterations_run"] == 300 and (w5["inlier"] == FILL).all()
    same(mt.Sim3Ransac(pr5, fill=FILL), w5, "best_inliers above every count")
    # 6. best_inliers equal to the top count: `>=` takes it
    pr6 = dict(pr, best_inliers=top, min_inliers=257)
    w6 = F.sim3_ransac_host(pr6, lib, fill=FILL)
    assert w6["selected"] == int(np.nonzero(c == top)[0][-1])
    same(mt.Sim3Ransac(pr6, fill=FILL), w6, "best_inliers equal to the top count")


def batch_problems(B):
    ns = [20, 0, 65, 2, 257, 10, 64, 1025, 3, 63, 33]
    nh = [20, 5, 300, 4, 3, 7, 1, 5, 0, 64, 65]
    out = []
    for b in range(B):
        n, h = ns[b % len(ns)], nh[b % len(nh)]
        if b >= len(ns):
            n, h = min(n, 65), min(h, 20)
        # problem 5 of every eleven has n = 10 < min_inliers = 20; problems with n = 0, n = 2 and n_hyp = 0 are not run either
        out.append(sc.problem(sized_case(n, h, b % 2 == 1, seed=b, min_inliers=20 if n == 10 else min(20, n // 3))))
    return out


def check_batch(lib, mt, B):
    prs = batch_problems(B)
    got = mt.Sim3RansacBatch(prs, fill=FILL)
    assert len(got) == B
    ran = 0
    for b in range(B):
        one = mt.Sim3Ransac(prs[b], fill=FILL)
        same(got[b], one, "problem %d of %d" % (b, B))
        n, h = prs[b]["n"], prs[b]["n_hyp"]
        if n < 3 or n < prs[b]["min_inliers"] or h == 0:
            assert one["selected"] == -1 and (one["inlier"] == FILL).all() and (one["counts"] == FILL).all(), b
            assert one["iterations_run"] == 0 and one["n_inliers"] == 0   # the structs start zeroed: not written
        else:
            ran += 1
    return ran


def check_errors(lib, mt):
    """every argument error: RGBL_ERR_INVALID, and every output of every problem stays as the caller left it"""
    base = sc.problem(sized_case(40, 5, False, seed=31))
    case = sized_case(40, 5, False, seed=31)
    pool = F.MapPointPool(16, lib=lib)

    def broken(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c
    bad = {"sample too large": broken("samples", (2, 1), 40),
           "sample negative": broken("samples", (0, 0), -1),
           "sample repeated": broken("samples", (4, 2), base["samples"][4, 0]),
           "K NaN": broken("K1", 1, np.nan),
           "K2 inf": broken("K2", 3, np.inf),
           "threshold NaN": broken("max_err2", 7, np.nan),
           "threshold inf": broken("max_err1", 0, np.inf),
           "n too large": dict(base, n=65536),
           "n_hyp negative": dict(base, n_hyp=-1),
           "n_hyp too large": dict(base, n_hyp=N_HYP_MAX + 1),
           "no points": dict({k: v for k, v in base.items() if k != "x2c"}),
           "no thresholds": dict({k: v for k, v in base.items() if k != "max_err1"}, n=40),
           "slot outside the pool": sc.pool_problem(case, pool, np.arange(40, dtype=np.int32), np.zeros(40, np.int32)),
           "pose NaN": sc.pool_problem(case, pool, np.zeros(40, np.int32), np.zeros(40, np.int32), tcw2=np.array([0, np.nan, 0], np.float32))}
    for what, pr in bad.items():
        for batch in (False, True):
            keep = []
            I, O = (L.Sim3Input * 2)(), (L.Sim3Output * 2)()
            F.ORBmatcher._sim3_input(base, keep, I[0])
            F.ORBmatcher._sim3_input(pr, keep, I[1])
            bufs = []
            for b in range(2):
                C.memset(C.byref(O[b]), 0x5a, C.sizeof(L.Sim3Output))
                n, nh = min(max(I[b].n, 0), 40), min(max(I[b].n_hyp, 0), 5)
                bufs.append((np.full(n, 9, np.uint8), np.full(nh, 9, np.int32), np.full((nh, 16), 9, np.float32)))
                O[b].inlier, O[b].counts, O[b].T12_all = [a.ctypes.data for a in bufs[b]]
            before = [bytes(O[0]), bytes(O[1])]
            if batch:   # the good problem in front of the bad one: neither is written
                rc = lib.rgbl_sim3_ransac_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))
            else:
                rc = lib.rgbl_sim3_ransac(mt.h, C.byref(I[1]), C.byref(O[1]))
            assert rc == L.ERR_INVALID, (what, batch, rc)
            if what in ("n too large", "n_hyp too large"):
                assert b"65535" in lib.rgbl_last_error() and b"%d" % N_HYP_MAX in lib.rgbl_last_error(), lib.rgbl_last_error()
            assert [bytes(O[0]), bytes(O[1])] == before, (what, batch)
            assert all((a == 9).all() for bb in bufs for a in bb), (what, batch)
            if not batch:   # the host build refuses the same things (and every pool)
                assert lib.rgbl_sim3_ransac_host(C.byref(I[1]), C.byref(O[1])) == L.ERR_INVALID, what
                assert bytes(O[1]) == before[1] and all((a == 9).all() for a in bufs[1]), what
    # two pools in one batch
    pool2 = F.MapPointPool(64, lib=lib)
    pool3 = F.MapPointPool(64, lib=lib)
    sl = np.arange(40, dtype=np.int32)
    keep = []
    I, O = (L.Sim3Input * 2)(), (L.Sim3Output * 2)()
    F.ORBmatcher._sim3_input(sc.pool_problem(case, pool2, sl, sl), keep, I[0])
    F.ORBmatcher._sim3_input(sc.pool_problem(case, pool3, sl, sl), keep, I[1])
    before = [bytes(O[0]), bytes(O[1])]
    assert lib.rgbl_sim3_ransac_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == L.ERR_INVALID
    assert [bytes(O[0]), bytes(O[1])] == before
    assert lib.rgbl_sim3_ransac(mt.h, None, None) == L.ERR_INVALID
    assert lib.rgbl_sim3_ransac_host(C.byref(I[0]), None) == L.ERR_INVALID
    for p in (pool, pool2, pool3):
        p.close()
    same(mt.Sim3Ransac(base), F.sim3_ransac_host(base, lib), "after the refused calls")


# ---- n <= 65535 correspondences, n_hyp <= 2^20 hypotheses ---------------------------------------------------------------------
N_MAX, N_HYP_MAX = 65535, 1 << 20
PER_POINT = ("x1c", "x2c", "max_err1", "max_err2", "planted_outlier", "Xw1", "Xw2")


def limit_n_problem(lib):
    """N_MAX correspondences; the selected hypothesis counts correspondences 32768 and 65534 (the last) as inliers, and the
    first sample names both.  Returns (problem, the host build's result)."""
    case = sized_case(N_MAX, 20, False, seed=7)
    good = np.nonzero(case["planted_outlier"] == 0)[0]
    for at, k in ((N_MAX - 1, 10), (32768, 11)):
        if case["planted_outlier"][at]:
            for key in PER_POINT:
                case[key][[at, good[k]]] = case[key][[good[k], at]]
    case["samples"][0] = (N_MAX - 1, 32768, int(good[12]))
    pr = sc.problem(case, min_inliers=N_MAX)      # runs through: the best of the twenty is selected
    want = F.sim3_ransac_host(pr, lib, fill=FILL)
    assert want["selected"] >= 0 and want["iterations_run"] == 20 and want["n_inliers"] >= floor_of(N_MAX), want["n_inliers"]
    assert want["inlier"][N_MAX - 1] == 1 and want["inlier"][32768] == 1 and want["counts"][0] > 0
    return pr, want


def floor_of(of):
    return -(-of // 20)      # 5 %, as geometry_checks.FLOOR


def check_limit_n(lib, mt):
    pr, want = limit_n_problem(lib)
    same(mt.Sim3Ransac(pr, fill=FILL), want, "%d correspondences" % N_MAX)
    return want["n_inliers"]


def check_limit_hyp(lib, mt, n=20):
    """N_HYP_MAX hypotheses of n correspondences, run through; the best triple once more as the last hypothesis: the later one wins
    a tie, so the selection is hypothesis 2^20 - 1"""
    case = sized_case(n, 1, False, seed=11, outlier_share=0.2)
    rng = np.random.default_rng(5)
    samples = np.ascontiguousarray(rng.permuted(np.tile(np.arange(n, dtype=np.int32), (N_HYP_MAX, 1)), axis=1)[:, :3])
    pr = sc.problem(case, samples=samples, n_hyp=N_HYP_MAX, min_inliers=n)
    first = F.sim3_ransac_host(pr, lib)
    samples[-1] = samples[int(np.argmax(first["counts"]))]
    want = F.sim3_ransac_host(pr, lib, fill=FILL)
    assert want["selected"] == N_HYP_MAX - 1 and want["iterations_run"] == N_HYP_MAX and want["converged"] == 0, want["selected"]
    assert want["n_inliers"] == want["counts"].max() >= 3 and (want["counts"][N_HYP_MAX // 2:] > 3).any()
    same(mt.Sim3Ransac(pr, fill=FILL), want, "%d hypotheses" % N_HYP_MAX)
    return want["n_inliers"]


def check_threads(lib, rounds=4):
    """the call next to other matcher calls from other threads, every thread on a handle of its own"""
    pr = sc.problem(sized_case(257, 64, False, seed=41))
    want = F.sim3_ransac_host(pr, lib)
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

    def solve():
        m = F.ORBmatcher(0.6, False, lib=lib)
        for r in range(rounds):
            same(m.Sim3Ransac(pr), want, "round %d next to searches" % r)
        m.close()

    def search():
        m = F.ORBmatcher(0.6, False, lib=lib)
        for r in range(rounds):
            assert np.array_equal(m.SearchForTriangulation(kfa, kfb, Fm, ep, sf, s2)[2], want_tri)
        m.close()
    threads = [threading.Thread(target=guarded(f)) for f in (solve, search, solve, search)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    m0.close()
    assert not errors, errors
