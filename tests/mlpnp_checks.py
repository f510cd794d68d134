"""rgbl_mlpnp_ransac / _batch / _host - MLPnPsolver (src/MLPnPsolver.cpp), every hypothesis of a call at once: the checks
tests/test_mlpnp_emu.py runs with the kernels under the SIMT emulator and tests/test_mlpnp_gpu.py on the MI355X.  The yardstick is
the HOST build of csrc/mlpnp_math.h in the same library (rgbl_mlpnp_ransac_host), bit for bit: every hypothesis's [R | t] in
fp64, counts, Gauss-Newton paths, found, no_more, n_inliers, iterations_run, refines, Tcw, the flags and the new state.
tests/test_mlpnp_math.py holds that host build to the float64 model of tests/mlpnp_model.py.  NaN entries are compared as NaN,
not by payload (the sign of a generated NaN is the machine's)."""
import ctypes as C
import threading

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import mlpnp_cases as mc

# the minimal set (6, 7), chunk edges of the ballots (63, 64, 65), the 256 work-items that expand the masks (255, 256, 257), a second round (300)
NS = (6, 7, 63, 64, 65, 255, 256, 257, 300)
# one wave, a part of a workgroup of four, several workgroups, the size of a real call
NHYPS = (1, 2, 35, 300)
FILL = 7
N_MAX, N_HYP_MAX, B_MAX = 65535, 1 << 20, 32767


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    a, b = a.reshape(-1), b.reshape(-1)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), (what, "NaN pattern")
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    assert np.array_equal(a[~nan].view(u), b[~nan].view(u)), (what, a[~nan][:8], b[~nan][:8])


def same(got, want, what):
    for k in ("found", "no_more", "n_inliers", "iterations_run", "refines", "best_inliers"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("Tcw", "best_Tcw", "Tcw_all"):
        if want[k] is not None:
            same_bits(got[k], want[k], (what, k))
    for k in ("counts", "gn_path", "inlier", "best_mask"):
        if want[k] is not None:
            assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:8])


def sized_case(N, n_hyp, seed=0, **kw):
    kw.setdefault("min_inliers", max(6, N // 2))
    return mc.make_mlpnp_case(N, n_hyp, seed=200 + 13 * N + n_hyp + seed, **kw)


def check_size(lib, mt, N, n_hyp):
    """device against host build, bit for bit; returns the host's result dict"""
    case = sized_case(N, n_hyp)
    pr = mc.problem(case)
    want = F.mlpnp_ransac_host(pr, lib, fill=FILL)
    got = mt.MLPnPRansac(pr, fill=FILL)
    same(got, want, "N %d, n_hyp %d" % (N, n_hyp))
    assert (want["counts"] >= 0).all() and (want["counts"] <= N).all()
    assert want["found"] == 0 or want["n_inliers"] == int(want["inlier"].sum())
    assert (want["inlier"][case["mp_index"] < 0] == (0 if want["found"] else FILL)).all()
    return want


def check_forms(lib, mt):
    """host arrays against a resident frame and a pool whose slots are not the point indices, single and in one batch"""
    out = 0
    for N in (65, 300):
        case = sized_case(N, 35, seed=3)
        pr = mc.problem(case)
        want = mt.MLPnPRansac(pr)
        n = len(case["mp_index"])
        fr = F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), case["xy"], case["octave"], np.full(n, -1, np.float32))
        pool = F.MapPointPool(1000, lib=lib)
        slot = np.random.default_rng(N).permutation(1000)[:N].astype(np.int32)
        pool.update(slot, world_pos=case["world_pos"])
        res = {k: v for k, v in pr.items() if k not in ("xy", "octave", "world_pos")}
        forms = [dict(res, device=fr, pool=pool, slot=slot), dict(res, device=fr, world_pos=case["world_pos"]),
                 dict(res, xy=case["xy"], octave=case["octave"], pool=pool, slot=slot)]
        for i, form in enumerate(forms):
            same(mt.MLPnPRansac(form), want, "form %d, N %d" % (i, N))
        for i, r in enumerate(mt.MLPnPRansacBatch(forms + [pr])):
            same(r, want, "batch of the forms, problem %d" % i)
        pool.close()
        fr.close()
        out += want["n_inliers"]
    return out


def check_planar(lib, mt):
    """exactly planar scenes (z == 0, coordinates on a grid: the third pivot of the uncentred planarity matrix is exactly 0).
    1. only the sample is planar: the first 12 correspondences of a scene that is not; 2. the whole scene.  The 9-column branch must have been taken: the same samples on the scene lifted off the plane give other poses."""
    case = sized_case(120, 4, seed=5, n_on_plane=12, outlier_share=0.0)
    samples = np.array([[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [11, 3, 7, 1, 9, 5], [0, 20, 40, 60, 80, 100]], np.int32)
    pr = mc.problem(case, samples=samples, min_inliers=6)
    want = F.mlpnp_ransac_host(pr, lib, fill=FILL)
    same(mt.MLPnPRansac(pr, fill=FILL), want, "planar samples in a scene that is not")
    lifted = mc.problem(case, samples=samples, min_inliers=6, world_pos=case["world_pos"] + np.float32([0, 0, 0.5]) * (case["world_pos"][:, 2:] == 0))
    other = F.mlpnp_ransac_host(lifted, lib)
    assert not np.array_equal(other["Tcw_all"][0], want["Tcw_all"][0])
    whole = sized_case(90, 35, seed=6, planar=True, min_inliers=6)
    pr2 = mc.problem(whole)
    want2 = F.mlpnp_ransac_host(pr2, lib, fill=FILL)
    assert want2["refines"] >= 1, "no hypothesis of the planar scene reached six inliers"
    same(mt.MLPnPRansac(pr2, fill=FILL), want2, "a planar scene")
    return want2["refines"]


def check_degenerate(lib, mt):
    """coincident 3-D points, points on a line through the world origin (rank 1: the 12-column branch), a true pose of exactly
    identity (rot2rodrigues of a trace that rounds past 3, or an exact identity, gives w = 0, where the Jacobian is NaN and the
    solve fails) and points behind the camera (no depth-sign test: they may be inliers)"""
    case = sized_case(40, 4, seed=9)
    wp, mp = case["world_pos"].copy(), case["mp_index"]
    rows = mp[case["feat"]]                                   # the map-side row of each correspondence
    wp[rows[1:6]] = wp[rows[0]]                               # correspondences 0 .. 5 coincide
    d = np.float32([0.5, 0.25, 1.0])
    for j in range(6):
        wp[rows[6 + j]] = np.float32(2 + j) * d               # 6 .. 11 on a line through the origin
    samples = np.array([[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [0, 6, 1, 7, 2, 8], case["samples"][0]], np.int32)
    pr = mc.problem(case, world_pos=wp, samples=samples, min_inliers=6)
    want = F.mlpnp_ransac_host(pr, lib, fill=FILL)
    same(mt.MLPnPRansac(pr, fill=FILL), want, "coincident and collinear samples")
    ident = sized_case(60, 35, seed=10, identity=True)
    pr2 = mc.problem(ident)
    want2 = F.mlpnp_ransac_host(pr2, lib, fill=FILL)
    same(mt.MLPnPRansac(pr2, fill=FILL), want2, "a true pose of exactly identity")
    assert want2["found"] == 1 and np.abs(want2["Tcw"] - np.eye(4)).max() < 1e-4
    exact = mc.problem(mc.make_exact_identity_case())
    want4 = F.mlpnp_ransac_host(exact, lib, fill=FILL)
    same(mt.MLPnPRansac(exact, fill=FILL), want4, "exact observations of an identity pose")
    at_zero = want4["gn_path"] == 32                          # w = 0: the first solve fails, x stays
    assert at_zero.sum() >= 5 and (want4["counts"][at_zero] == 40).all(), want4["gn_path"]
    assert np.array_equal(want4["Tcw_all"][at_zero][:, :, :3], np.tile(np.eye(3), (int(at_zero.sum()), 1, 1)))
    assert want4["found"] == 1 and want4["n_inliers"] == 40
    behind = sized_case(60, 35, seed=11, n_behind=8, outlier_share=0.0)
    pr3 = mc.problem(behind)
    want3 = F.mlpnp_ransac_host(pr3, lib, fill=FILL)
    same(mt.MLPnPRansac(pr3, fill=FILL), want3, "points behind the camera")
    assert want3["found"] == 1 and want3["inlier"][behind["feat"][-8:]].sum() > 0, "no point behind the camera is an inlier"
    return want, want2, want3


def check_scan(lib, mt):
    """the stop rule on crafted sample sequences; every expectation is asserted on the host build, then the device must equal it.
    Refine as the reference compiles it returns the current hypothesis: it succeeds iff c[k] > min_inliers."""
    case = sized_case(100, 300, seed=21, outlier_share=0.35)
    pr = mc.problem(case)
    S, N = case["samples"], case["N"]
    c = F.mlpnp_ransac_host(dict(pr, min_inliers=100), lib)["counts"]       # runs through: every count
    done = []

    def both(p, what):
        want = F.mlpnp_ransac_host(p, lib, fill=FILL)
        same(mt.MLPnPRansac(p, fill=FILL), want, what)
        done.append(what)
        return want

    def pose(r, h):
        return r["Tcw_all"][h].astype(np.float32)
    order = np.argsort(c, kind="stable")
    mid = order[(c[order] >= 8) & (c[order] < c.max())]
    assert len(mid) >= 2, "no hypothesis with a count between 8 and the top"
    k, top = int(mid[0]), int(np.argmax(c))
    j = int(np.nonzero(c > c[k])[0][0])
    low = int(np.nonzero(c < c[k])[0][0])
    # 1. c[k] == min_inliers qualifies but Refine fails (strict); min_inliers one lower succeeds with the same hypothesis
    eq = both(dict(pr, samples=S[[k]], n_hyp=1, min_inliers=int(c[k])), "count == min_inliers")
    assert (eq["found"], eq["no_more"], eq["refines"], eq["n_inliers"], eq["iterations_run"], eq["best_inliers"]) == (1, 1, 1, int(c[k]), 1, int(c[k])), eq
    assert np.array_equal(eq["Tcw"], eq["best_Tcw"]) and np.array_equal(eq["Tcw"][:3], pose(eq, 0))
    lo = both(dict(pr, samples=S[[k]], n_hyp=1, min_inliers=int(c[k]) - 1), "count == min_inliers + 1")
    assert (lo["found"], lo["no_more"], lo["refines"], lo["n_inliers"]) == (1, 0, 1, int(c[k])), lo
    assert np.array_equal(lo["Tcw"], eq["Tcw"]) and np.array_equal(lo["inlier"], eq["inlier"]) and int(lo["inlier"].sum()) == c[k]
    # 2. a record whose Refine fails, a hypothesis that does not qualify, then a record whose Refine succeeds
    two = both(dict(pr, samples=S[[k, low, j]], n_hyp=3, min_inliers=int(c[k])), "a failed Refine, then a success")
    assert (two["found"], two["no_more"], two["refines"], two["iterations_run"], two["n_inliers"], two["best_inliers"]) == (1, 0, 2, 3, int(c[j]), int(c[j])), two
    assert np.array_equal(two["Tcw"][:3], pose(two, 2)) and np.array_equal(two["best_Tcw"], two["Tcw"])
    # 3. ties: `>` keeps the first record; every qualifying hypothesis calls Refine
    rep = both(dict(pr, samples=S[[k, k, k]], n_hyp=3, min_inliers=int(c[k])), "equal counts: the first is the record")
    assert (rep["refines"], rep["no_more"], rep["iterations_run"], rep["best_inliers"]) == (3, 1, 3, int(c[k]))
    # 4. a run-through without any qualifying hypothesis
    none = both(dict(pr, min_inliers=100), "a run-through with none")
    assert (none["found"], none["no_more"], none["n_inliers"], none["iterations_run"], none["refines"], none["best_inliers"]) == (0, 1, 0, 300, 0, 0)
    assert np.array_equal(none["Tcw"], np.eye(4, dtype=np.float32)) and (none["inlier"] == FILL).all() and (none["best_mask"] == FILL).all()
    # 5. a larger record carried in from an earlier call: a success returns the CURRENT hypothesis, which is not the record
    first = both(dict(pr, samples=S[[top]], n_hyp=1, min_inliers=int(c[top])), "the call that leaves the state")
    assert (first["found"], first["no_more"], first["best_inliers"]) == (1, 1, int(c[top]))
    state = dict(best_inliers=first["best_inliers"], best_mask=first["best_mask"][:N], best_Tcw=first["best_Tcw"])
    second = both(dict(pr, samples=S[[low, j]], n_hyp=2, min_inliers=int(c[k]), **state), "a success below the carried record")
    assert c[k] < c[j] < c[top]
    assert (second["found"], second["no_more"], second["refines"], second["iterations_run"], second["n_inliers"], second["best_inliers"]) == (1, 0, 1, 2, int(c[j]), int(c[top]))
    assert np.array_equal(second["Tcw"][:3], pose(second, 1)) and not np.array_equal(second["Tcw"], first["Tcw"])
    assert np.array_equal(second["best_mask"], first["best_mask"]) and np.array_equal(second["best_Tcw"], first["best_Tcw"])
    # ... and a run-through under it hands out the carried pose and mask
    third = both(dict(pr, samples=S[[low, k]], n_hyp=2, min_inliers=int(c[k]), **state), "a run-through under the carried record")
    assert (third["found"], third["no_more"], third["refines"], third["n_inliers"]) == (1, 1, 1, int(c[top]))
    assert np.array_equal(third["Tcw"], first["best_Tcw"]) and np.array_equal(third["inlier"], first["inlier"])
    # 6. the `||` of the loop condition: mRansacMinInliers == N gives mRansacMaxIts = 1, yet iterate(5) runs 5 iterations
    mn, its = mc.ransac_parameters(12, min_inliers=12)
    assert (mn, its) == (12, 1) and mc.calls_n_hyp(its, 0, 5) == 5 and mc.calls_n_hyp(300, 298, 5) == 5 and mc.calls_n_hyp(300, 0, 5) == 300
    small = sized_case(12, 5, seed=22, min_inliers=12)
    five = both(mc.problem(small), "min_inliers == N")
    assert five["iterations_run"] == 5 and five["no_more"] == 1     # a count cannot exceed N = min_inliers
    return done


def batch_problems(B):
    Ns = [20, 6, 65, 300, 257, 10, 64, 40, 7, 63, 33]
    nh = [20, 5, 35, 4, 3, 7, 1, 5, 0, 64, 65]
    out = []
    for b in range(B):
        N, h = Ns[b % len(Ns)], nh[b % len(nh)]
        if b >= len(Ns):
            N, h = min(N, 65), min(h, 20)
        # problem 5 of every eleven has N = 10 < min_inliers = 20; problem 8 has no hypothesis
        out.append(mc.problem(sized_case(N, h, seed=b, min_inliers=20 if N == 10 else max(6, N // 2))))
    return out


def check_batch(lib, mt, B):
    prs = batch_problems(B)
    got = mt.MLPnPRansacBatch(prs, fill=FILL)
    assert len(got) == B
    ran = 0
    for b in range(B):
        one = mt.MLPnPRansac(prs[b], fill=FILL)
        same(got[b], one, "problem %d of %d" % (b, B))
        N, h = int((prs[b]["mp_index"] >= 0).sum()), prs[b]["n_hyp"]
        if N < prs[b]["min_inliers"] or h == 0:
            assert (one["found"], one["no_more"], one["n_inliers"], one["iterations_run"]) == (0, int(N < prs[b]["min_inliers"]), 0, 0), b
            assert (one["inlier"] == FILL).all() and (one["counts"] == FILL).all() and np.array_equal(one["Tcw"], np.eye(4, dtype=np.float32)), b
        else:
            ran += 1
    return ran


def check_errors(lib, mt):
    """every argument error: RGBL_ERR_INVALID, and every output of every problem stays as the caller left it"""
    case = sized_case(40, 5, seed=31)
    base = mc.problem(case)
    N = case["N"]
    pool = F.MapPointPool(16, lib=lib)
    n = len(case["mp_index"])
    fr = F.DeviceFrame(n + 5, lib=lib).upload(np.zeros((n + 5, 32), np.uint8), np.zeros((n + 5, 2), np.float32), np.zeros(n + 5, np.int32))

    def broken(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c
    first = int(case["feat"][0])
    mask = np.zeros(N, np.uint8)
    mask[:7] = 1
    bad = {"sample too large": broken("samples", (2, 1), N),
           "sample negative": broken("samples", (0, 0), -1),
           "sample repeated": broken("samples", (4, 5), base["samples"][4, 0]),
           "K NaN": broken("K", 1, np.nan),
           "th2 inf": dict(base, th2=np.inf),
           "sigma2 NaN": broken("level_sigma2", 3, np.nan),
           "n too large": dict(base, n=N_MAX + 1),
           "n_hyp negative": dict(base, n_hyp=-1),
           "n_hyp too large": dict(base, n_hyp=N_HYP_MAX + 1),
           "min_inliers 5": dict(base, min_inliers=5),
           "mp_index too large": broken("mp_index", first, N),
           "mp_index -2": broken("mp_index", first, -2),
           "octave too large": broken("octave", first, 8),
           "octave negative": broken("octave", first, -1),
           "n_levels 0": dict(base, n_levels=0),
           "n_levels 17": dict(base, n_levels=17),
           "no points": {k: v for k, v in base.items() if k != "world_pos"} | dict(n_points=N),
           "no frame": {k: v for k, v in base.items() if k != "xy"},
           "no samples": dict({k: v for k, v in base.items() if k != "samples"}, n_hyp=5),
           "no sigma2": dict({k: v for k, v in base.items() if k != "level_sigma2"}, n_levels=8),
           "best_inliers without a mask": dict(base, best_inliers=7),
           "best_inliers that is not the mask's": dict(base, best_inliers=8, best_mask=mask),
           "best_inliers negative": dict(base, best_inliers=-1),
           "slot outside the pool": mc.pool_problem(case, pool, np.arange(N, dtype=np.int32)),
           "frame of another size": dict({k: v for k, v in base.items() if k not in ("xy", "octave")}, device=fr)}
    for what, pr in bad.items():
        for batch in (False, True):
            keep = []
            I, O = (L.MlpnpInput * 2)(), (L.MlpnpOutput * 2)()
            F.ORBmatcher._mlpnp_input(base, keep, I[0])
            F.ORBmatcher._mlpnp_input(pr, keep, I[1])
            bufs = []
            for b in range(2):
                C.memset(C.byref(O[b]), 0x5a, C.sizeof(L.MlpnpOutput))
                nn, nh = min(max(I[b].n, 0), n), min(max(I[b].n_hyp, 0), 5)
                bufs.append((np.full(nn, 9, np.uint8), np.full(nn, 9, np.uint8), np.full(nh, 9, np.int32), np.full((nh, 12), 9, np.float64), np.full(nh, 9, np.int32)))
                O[b].inlier, O[b].best_mask, O[b].counts, O[b].Tcw_all, O[b].gn_path = [a.ctypes.data for a in bufs[b]]
            before = [bytes(O[0]), bytes(O[1])]
            if batch:   # the good problem in front of the bad one: neither is written
                rc = lib.rgbl_mlpnp_ransac_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))
            else:
                rc = lib.rgbl_mlpnp_ransac(mt.h, C.byref(I[1]), C.byref(O[1]))
            assert rc == L.ERR_INVALID, (what, batch, rc)
            assert [bytes(O[0]), bytes(O[1])] == before, (what, batch)
            assert all((a == 9).all() for bb in bufs for a in bb), (what, batch)
            if not batch:   # the host build refuses the same things (and every pool and resident frame)
                assert lib.rgbl_mlpnp_ransac_host(C.byref(I[1]), C.byref(O[1])) == L.ERR_INVALID, what
                assert bytes(O[1]) == before[1] and all((a == 9).all() for a in bufs[1]), what
    # two pools in one batch
    pool2, pool3 = F.MapPointPool(64, lib=lib), F.MapPointPool(64, lib=lib)
    sl = np.arange(N, dtype=np.int32)
    keep = []
    I, O = (L.MlpnpInput * 2)(), (L.MlpnpOutput * 2)()
    F.ORBmatcher._mlpnp_input(mc.pool_problem(case, pool2, sl), keep, I[0])
    F.ORBmatcher._mlpnp_input(mc.pool_problem(case, pool3, sl), keep, I[1])
    before = [bytes(O[0]), bytes(O[1])]
    assert lib.rgbl_mlpnp_ransac_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == L.ERR_INVALID
    assert [bytes(O[0]), bytes(O[1])] == before
    assert lib.rgbl_mlpnp_ransac(mt.h, None, None) == L.ERR_INVALID
    assert lib.rgbl_mlpnp_ransac_host(C.byref(I[0]), None) == L.ERR_INVALID
    for p in (pool, pool2, pool3):
        p.close()
    fr.close()
    same(mt.MLPnPRansac(base), F.mlpnp_ransac_host(base, lib), "after the refused calls")


def check_limits(lib, mt):
    """every size limit from both sides: the highest value is accepted and computed, one past it is refused (check_errors holds
    the refusals of n, n_hyp, min_inliers, n_levels, the sample, mp_index and octave ranges)"""
    case = sized_case(40, 5, seed=33)
    N = case["N"]
    base = mc.problem(case)

    def set_at(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c
    first = int(case["feat"][0])
    sig16 = (np.float32(1.2) ** np.arange(16, dtype=np.float32)) ** 2
    inside = {"sample N - 1": set_at("samples", (2, 1), N - 1) if N - 1 not in base["samples"][2] else base,
              "octave n_levels - 1": set_at("octave", first, 7),
              "n_levels 16, octave 15": dict(set_at("octave", first, 15), level_sigma2=sig16),
              "n_levels 1": dict(base, octave=np.zeros_like(base["octave"]), level_sigma2=sig16[:1]),
              "min_inliers 6": dict(base, min_inliers=6),
              "mp_index n_points - 1 only": base}
    for what, pr in inside.items():
        same(mt.MLPnPRansac(pr, fill=FILL), F.mlpnp_ransac_host(pr, lib, fill=FILL), what)
    # a slot at capacity - 1
    pool = F.MapPointPool(N, lib=lib)
    slot = np.arange(N, dtype=np.int32)[::-1].copy()
    pool.update(slot, world_pos=case["world_pos"])
    same(mt.MLPnPRansac(mc.pool_problem(case, pool, slot)), mt.MLPnPRansac(base), "slot capacity - 1")
    keep = []
    I, O = F.ORBmatcher._mlpnp_input(mc.pool_problem(case, pool, slot + 1), keep), L.MlpnpOutput()
    assert lib.rgbl_mlpnp_ransac(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"slot" in lib.rgbl_last_error()
    pool.close()
    # n_hyp = 2^20 is inside (a problem with N < min_inliers runs nothing), 2^20 + 1 is refused in the same problem
    few = dict(base, min_inliers=N + 1, samples=None)
    r = mt.MLPnPRansac(dict(few, n_hyp=N_HYP_MAX), diag=False)
    assert (r["found"], r["no_more"]) == (0, 1)
    keep = []
    I = F.ORBmatcher._mlpnp_input(dict(few, n_hyp=N_HYP_MAX + 1), keep)
    assert lib.rgbl_mlpnp_ransac(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"%d" % N_HYP_MAX in lib.rgbl_last_error()
    # the masks of one call: n_hyp x ceil(N / 64) words over all problems may not exceed 2^26 (each maximum alone stays inside:
    # check_limit_n, check_limit_hyp); 2^20 hypotheses of 65 words are refused before anything is staged
    big = mc.problem(sized_case(64 * 64 + 1, 1, seed=34, extra_features=0, min_inliers=6))
    keep = []
    I = F.ORBmatcher._mlpnp_input(dict(big, samples=np.tile(big["samples"], (N_HYP_MAX, 1)), n_hyp=N_HYP_MAX), keep)
    assert lib.rgbl_mlpnp_ransac(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"mask words" in lib.rgbl_last_error()
    # n_problems: 32767 problems that run nothing are inside, 32768 are refused
    keep = []
    I, O = (L.MlpnpInput * (B_MAX + 1))(), (L.MlpnpOutput * (B_MAX + 1))()
    F.ORBmatcher._mlpnp_input(dict(few, n_hyp=0), keep, I[0])
    for b in range(1, B_MAX + 1):
        C.memmove(C.byref(I[b]), C.byref(I[0]), C.sizeof(L.MlpnpInput))
    assert lib.rgbl_mlpnp_ransac_batch(mt.h, B_MAX, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == 0
    assert O[B_MAX - 1].no_more == 1 and O[B_MAX].no_more == 0
    assert lib.rgbl_mlpnp_ransac_batch(mt.h, B_MAX + 1, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == L.ERR_INVALID


def limit_n_problem(lib):
    """a frame of N_MAX features, every one with a map point; the first sample names correspondence N_MAX - 1 and 32768.
    Returns (problem, the host build's result)."""
    case = sized_case(N_MAX, 3, seed=7, extra_features=0, min_inliers=N_MAX // 2)
    good = np.nonzero(case["planted_outlier"] == 0)[0]
    picks = [int(g) for g in good if g not in (N_MAX - 1, 32768)][:4]
    case["samples"][0] = [N_MAX - 1, 32768] + picks
    pr = mc.problem(case)
    want = F.mlpnp_ransac_host(pr, lib, fill=FILL)
    assert want["iterations_run"] >= 1 and want["counts"].max() <= N_MAX
    return pr, want


def check_limit_n(lib, mt):
    pr, want = limit_n_problem(lib)
    same(mt.MLPnPRansac(pr, fill=FILL), want, "%d correspondences" % N_MAX)
    keep = []
    I, O = F.ORBmatcher._mlpnp_input(dict(pr, n=N_MAX + 1), keep), L.MlpnpOutput()
    assert lib.rgbl_mlpnp_ransac(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"65535" in lib.rgbl_last_error()
    return want["counts"].max()


def check_limit_hyp(lib, mt, N=20):
    """N_HYP_MAX hypotheses, run through (min_inliers = N, one planted outlier more than none): 64 distinct samples, repeated;
    the host build computes the 64, every repetition on the device must carry the same bits"""
    case = sized_case(N, 64, seed=11, outlier_share=0.3, min_inliers=N)
    assert case["planted_outlier"].sum() > 0
    pr64 = mc.problem(case)
    want = F.mlpnp_ransac_host(pr64, lib)
    assert want["found"] == 0 and want["iterations_run"] == 64
    rep = N_HYP_MAX // 64
    got = mt.MLPnPRansac(dict(pr64, samples=np.tile(case["samples"], (rep, 1)), n_hyp=N_HYP_MAX))
    assert (got["found"], got["no_more"], got["iterations_run"]) == (0, 1, N_HYP_MAX)
    assert np.array_equal(got["counts"].reshape(rep, 64), np.tile(want["counts"], (rep, 1)))
    same_bits(got["Tcw_all"][-64:], want["Tcw_all"], "the last 64 hypotheses")
    same_bits(got["Tcw_all"][:64], want["Tcw_all"], "the first 64 hypotheses")
    return int(want["counts"].max())


def check_threads(lib, rounds=4):
    """the call next to other matcher calls from other threads, every thread on a handle of its own"""
    pr = mc.problem(sized_case(257, 35, seed=41))
    want = F.mlpnp_ransac_host(pr, lib)
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
            same(m.MLPnPRansac(pr), want, "round %d next to searches" % r)
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
