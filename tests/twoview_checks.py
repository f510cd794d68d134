"""rgbl_two_view_reconstruct / _batch / _host - TwoViewReconstruction (src/TwoViewReconstruction.cc), every homography and
fundamental hypothesis of a call at once: the checks tests/test_twoview_emu.py runs with the kernels under the SIMT emulator and
tests/test_twoview_gpu.py on the MI355X.  The yardstick is the HOST build of csrc/twoview_math.h in the same library
(rgbl_two_view_reconstruct_host), bit for bit: every hypothesis's score and model, both winners and their masks, the choice, the
exit taken, n_good, parallax, T21, the points and the flags.  NaN entries are compared as NaN, not by payload (the sign of a
generated NaN is the machine's).  The expectations about WHICH exit a scene takes were read off the host build once and are
asserted on it; the device then has to equal the host build."""
import ctypes as C
import threading

import numpy as np

from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import cases
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import twoview_cases as tc

# the minimal set (8, 9), the chunk edges of the ballots and of the serial sum (63, 64, 65), a real call's minimum (100), the 256
# work-items of CheckRT (257)
NS = (8, 9, 63, 64, 65, 100, 257)
# one wave, a part of a workgroup of four, exactly one, one more, the reference's 200
NHYPS = (1, 3, 4, 5, 200)
FILL = 7
N_MAX, N_HYP_MAX, B_MAX = 65535, 1 << 20, 32767
FOUND, NO_SCORE, H_RATIO, H_RULE, F_FEW_OR_SIMILAR, F_PARALLAX = range(6)
INTS = ("found", "model", "exit_code", "best_h", "best_f", "p3d_assigned", "n_inliers", "best_motion", "aux")
FLOATS = ("SH", "SF", "H21", "F21", "R21", "t21", "parallax", "p3d", "scores", "models")
ARRAYS = ("n_good", "triangulated", "inliers_h", "inliers_f")


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    a, b = a.reshape(-1), b.reshape(-1)
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), (what, "NaN pattern")
    assert np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)), (what, a[~nan][:8], b[~nan][:8])


def same(got, want, what):
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in FLOATS:
        if want[k] is not None:
            same_bits(got[k], want[k], (what, k))
    for k in ARRAYS:
        if want[k] is not None:
            assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0][:8])


def consistent(pr, w, what):
    """what must hold of any result, whatever the scene"""
    first, _ = tc.matches(pr)
    N, n1 = len(first), len(pr["matches12"])
    assert w["model"] in (-1, 0, 1) and w["found"] in (0, 1), what
    assert (w["exit_code"] == FOUND) == (w["found"] == 1), what
    assert (w["model"] == -1) == (w["exit_code"] == NO_SCORE), what
    assert w["p3d_assigned"] == (1 if w["found"] and w["model"] == 1 else 0), what
    if w["scores"] is not None and len(w["scores"]):
        for md, (best, S) in enumerate(((w["best_h"], w["SH"]), (w["best_f"], w["SF"]))):
            sc = w["scores"][:, md]
            top = np.nanmax(np.where(np.isnan(sc), 0, sc))
            if top > 0:     # the first strictly greater score: the first occurrence of the maximum; a NaN never wins
                assert best == int(np.nonzero(sc == top)[0][0]) and S == top, (what, md, best, S, top)
            else:
                assert best == -1 and S == 0, (what, md)
    if w["model"] >= 0:
        mask = (w["inliers_h"] if w["model"] == 0 else w["inliers_f"])[:N]
        assert w["n_inliers"] == int(mask.sum()), what
        if w["found"]:
            assert (w["triangulated"][np.setdiff1d(np.arange(n1), first[mask == 1])] == 0).all(), (what, "a flag on a key that is no inlier")
            assert int(w["triangulated"].sum()) <= w["n_good"][w["best_motion"]], what
        else:
            assert (w["triangulated"] == FILL).all() and (w["p3d"] == FILL).all(), (what, "written without a solution")
    if w["best_f"] < 0 and w["inliers_f"] is not None:
        assert (w["inliers_f"] == FILL).all(), (what, "the F mask is empty in the reference when no F hypothesis scores")


def both(lib, mt, pr, what):
    want = F.two_view_reconstruct_host(pr, lib, fill=FILL)
    got = mt.TwoViewReconstruct(pr, fill=FILL)
    same(got, want, what)
    consistent(pr, want, what)
    return want


def sized_case(N, n_hyp, seed=0, **kw):
    kw.setdefault("pixel_noise", 0.1)
    return tc.make_two_view_case(N, n_hyp, seed=300 + 11 * N + n_hyp + seed, **kw)


def check_size(lib, mt, N, n_hyp):
    """device against host build, bit for bit; n1 != n2 and unmatched keys lie between the matched ones"""
    case = sized_case(N, n_hyp)
    pr = tc.problem(case)
    assert len(pr["xy1"]) != len(pr["xy2"]) and (pr["matches12"][:-1] < 0).any()
    want = both(lib, mt, pr, "N %d, n_hyp %d" % (N, n_hyp))
    assert want["scores"].shape == (n_hyp, 2)
    return want


def doubled(case, at=(3, 30, 60, 90)):
    """four matches whose keys lie exactly where their neighbours' do, and the set of those eight: four distinct points fix a
    homography, while the 8 x 9 matrix of the fundamental system has rank 4 - its null vector is one of many and F21 fits little"""
    first, second = tc.matches(case)
    xy1, xy2 = case["xy1"].copy(), case["xy2"].copy()
    for p in at:
        xy1[first[p + 1]] = xy1[first[p]]
        xy2[second[p + 1]] = xy2[second[p]]
    samples = np.array([[q for p in at for q in (p, p + 1)]], np.int32)
    return tc.problem(case, xy1=xy1, xy2=xy2, samples=samples, n_hyp=1)


def scene_problems():
    """(name, problem, model, exit): every scene type, both models, every `return false` of Reconstruct / ReconstructF / ReconstructH"""
    mk = tc.make_two_view_case
    out = []
    for seed in (0, 3):
        out.append(("general %d" % seed, tc.problem(mk(100, 200, seed=seed, scene="general", pixel_noise=0.1)), 1, FOUND))
    out.append(("forward", tc.problem(mk(100, 200, seed=0, scene="forward", pixel_noise=0.1)), 1, FOUND))
    out.append(("forward without parallax", tc.problem(mk(100, 200, seed=4, scene="forward", pixel_noise=0.1)), 1, F_PARALLAX))
    out.append(("mirror: nsimilar 2", tc.problem(mk(100, 2, seed=0, scene="mirror", pixel_noise=0.0, outlier_share=0.0)), 1, F_FEW_OR_SIMILAR))
    out.append(("rotation through F: nsimilar 2", tc.problem(mk(100, 2, seed=0, scene="rotation", pixel_noise=0.0, outlier_share=0.0)), 1, F_FEW_OR_SIMILAR))
    out.append(("outliers: too few", tc.problem(mk(100, 200, seed=0, scene="outliers")), 1, F_FEW_OR_SIMILAR))
    out.append(("planar", tc.problem(mk(100, 5, seed=0, scene="planar", pixel_noise=0.1, outlier_share=0.0)), 0, FOUND))
    out.append(("planar, doubled set", doubled(mk(100, 1, seed=0, scene="planar", pixel_noise=0.0, outlier_share=0.0)), 0, FOUND))
    out.append(("planar, second best too good", tc.problem(mk(100, 2, seed=4, scene="planar", pixel_noise=0.1, outlier_share=0.0)), 0, H_RULE))
    out.append(("rotation through H: no parallax", tc.problem(mk(100, 2, seed=0, scene="rotation", pixel_noise=0.1, outlier_share=0.0)), 0, H_RULE))
    out.append(("exact rotation, doubled set: d1 == d2", doubled(mk(100, 1, seed=0, scene="rotation", pixel_noise=0.0, outlier_share=0.0)), 0, H_RATIO))
    exact = mk(100, 5, seed=1, scene="general", pixel_noise=0.0, outlier_share=0.0)
    out.append(("sigma 0.01: SH == 0", tc.problem(exact, sigma=np.float32(0.01)), 1, FOUND))
    out.append(("sigma 0: SH + SF == 0", tc.problem(mk(100, 5, seed=1, scene="general", pixel_noise=0.3), sigma=np.float32(0.0)), -1, NO_SCORE))
    return out


def check_scenes(lib, mt):
    taken = {}
    for name, pr, model, code in scene_problems():
        want = both(lib, mt, pr, name)
        assert (want["model"], want["exit_code"]) == (model, code), (name, want["model"], want["exit_code"], want["aux"], want["n_good"], want["parallax"])
        taken.setdefault((model, code), []).append(name)
        if name.startswith("mirror") or name.startswith("rotation through F"):
            assert want["aux"] == 2 and want["n_good"].max() >= 90, (name, want["aux"], want["n_good"])     # not `too few`: nsimilar
        if name.startswith("outliers"):
            assert want["aux"] <= 1 and want["n_good"].max() < 50, (name, want["n_good"])
        if name.startswith("sigma 0.01"):
            assert want["SH"] == 0 and want["best_h"] == -1 and not want["H21"].any() and want["SF"] > 0, name
        if name.startswith("sigma 0:"):
            assert want["SH"] == 0 and want["SF"] == 0 and (want["n_good"] == 0).all(), name
        if model == 0 and code == FOUND:
            # ReconstructH drops bestP3D: the reference's vP3D is not assigned, the winner's points are handed out all the same
            assert want["p3d_assigned"] == 0 and want["triangulated"].sum() > 50 and np.abs(want["p3d"][want["triangulated"] == 1]).max() > 0, name
            assert want["aux"] < 0.75 * want["n_good"][want["best_motion"]] and want["parallax"][want["best_motion"]] >= 1.0, name
        if code == FOUND:
            R = want["R21"].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-5 and np.linalg.det(R) > 0.999 and abs(np.linalg.norm(want["t21"]) - 1) < 1e-5, name
        if code == F_PARALLAX:
            assert want["aux"] == 1 and want["parallax"][want["best_motion"]] <= 1.0, name
        if code == H_RATIO:
            assert (want["n_good"] == 0).all() and want["best_motion"] == -1, name
    return taken


def check_degenerate(lib, mt):
    """sets of coincident points and of points on a line in both frames: A has rank 2 / rank-deficient, the null vector is one of
    many, the model fits its own set and little else - whatever it scores, device and host build agree and the winner is the first
    strictly greater score (consistent()).  Then a frame whose keys share one x: meanDevX = 0, sX = 1.0 / 0 = inf, every model and
    every score is NaN, and a NaN never wins: SH = SF = 0, the first exit."""
    case = sized_case(60, 1, seed=5, outlier_share=0.0)
    first, second = tc.matches(case)
    xy1, xy2 = case["xy1"].copy(), case["xy2"].copy()
    for j in range(1, 8):                                   # matches 0 .. 7 coincide
        xy1[first[j]], xy2[second[j]] = xy1[first[0]], xy2[second[0]]
    for j in range(8):                                      # matches 8 .. 15 on a line
        xy1[first[8 + j]] = np.float32([100 + 30 * j, 50 + 15 * j])
        xy2[second[8 + j]] = np.float32([120 + 32 * j, 60 + 16 * j])
    samples = np.array([np.arange(8), np.arange(8, 16), np.arange(20, 28)], np.int32)
    pr = tc.problem(case, xy1=xy1, xy2=xy2, samples=samples, n_hyp=3)
    want = both(lib, mt, pr, "coincident and collinear sets")
    for k in (0, 1, 2):
        both(lib, mt, dict(pr, samples=samples[[k]], n_hyp=1), "set %d alone" % k)
    flat = xy2.copy()
    flat[:, 0] = np.float32(321.5)
    nan = both(lib, mt, dict(pr, xy2=flat), "the keys of frame 2 share one x")
    assert np.isnan(nan["scores"]).all() and np.isnan(nan["models"]).all(), nan["scores"]
    assert (nan["SH"], nan["SF"], nan["best_h"], nan["best_f"], nan["model"], nan["exit_code"]) == (0, 0, -1, -1, -1, NO_SCORE)
    return want


def check_ties(lib, mt):
    """equal scores: duplicated sets, the first wins (`currentScore > score`); equal nGood: the two mirror hypotheses of an
    exact rotation count every match (no depth test without parallax), nsimilar = 2"""
    case = sized_case(100, 4, seed=6)
    s = case["samples"]
    pr = tc.problem(case, samples=s[[0, 0, 1, 1, 2, 2, 3, 3]], n_hyp=8)
    want = both(lib, mt, pr, "every set twice")
    assert np.array_equal(want["scores"][0::2].view(np.uint32), want["scores"][1::2].view(np.uint32))
    assert want["best_h"] % 2 == 0 and want["best_f"] % 2 == 0, (want["best_h"], want["best_f"])
    rot = tc.problem(tc.make_two_view_case(100, 2, seed=0, scene="rotation", pixel_noise=0.0, outlier_share=0.0))
    tie = both(lib, mt, rot, "equal nGood")
    g = np.sort(tie["n_good"][:4])
    assert g[3] == g[2] == 100 and tie["aux"] == 2 and tie["exit_code"] == F_FEW_OR_SIMILAR, tie["n_good"]
    return want


def resident(lib, xy):
    n = len(xy)
    return F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), xy, np.zeros(n, np.int32), np.full(n, -1, np.float32))


def check_forms(lib, mt):
    """host arrays against resident frames, single and in one batch"""
    out = 0
    for N in (65, 257):
        case = sized_case(N, 20, seed=3)
        pr = tc.problem(case)
        want = mt.TwoViewReconstruct(pr)
        fr1, fr2 = resident(lib, case["xy1"]), resident(lib, case["xy2"])
        res = {k: v for k, v in pr.items() if k not in ("xy1", "xy2")}
        res.update(n1=len(case["xy1"]), n2=len(case["xy2"]))
        forms = [dict(res, device1=fr1, device2=fr2), dict(res, device1=fr1, xy2=case["xy2"]), dict(res, xy1=case["xy1"], device2=fr2)]
        for i, form in enumerate(forms):
            same(mt.TwoViewReconstruct(form), want, "form %d, N %d" % (i, N))
        for i, r in enumerate(mt.TwoViewReconstructBatch(forms + [pr])):
            same(r, want, "batch of the forms, problem %d" % i)
        fr1.close()
        fr2.close()
        out += want["n_inliers"]
    return out


def batch_problems(B):
    Ns = [20, 8, 65, 100, 257, 10, 64, 40, 9, 63, 33]
    nh = [20, 5, 35, 4, 3, 7, 1, 5, 0, 64, 65]
    scenes = ["general", "planar", "forward", "general", "rotation", "mirror", "general", "outliers"]
    out = []
    for b in range(B):
        N, h = Ns[b % len(Ns)], nh[b % len(nh)]
        if b >= len(Ns):
            N, h = min(N, 65), min(h, 20)
        out.append(tc.problem(sized_case(N, h, seed=b, scene=scenes[b % len(scenes)])))     # problem 8 of every eleven has no hypothesis
    return out


def check_batch(lib, mt, B):
    prs = batch_problems(B)
    got = mt.TwoViewReconstructBatch(prs, fill=FILL)
    assert len(got) == B
    ran = 0
    for b in range(B):
        one = mt.TwoViewReconstruct(prs[b], fill=FILL)
        same(got[b], one, "problem %d of %d" % (b, B))
        if prs[b]["n_hyp"] == 0:
            assert (one["found"], one["model"], one["exit_code"], one["best_h"], one["best_f"]) == (0, -1, NO_SCORE, -1, -1), b
            assert (one["p3d"] == FILL).all() and (one["inliers_h"] == FILL).all() and one["SH"] == 0 and one["SF"] == 0, b
        else:
            ran += 1
    return ran


def check_errors(lib, mt):
    """every argument error: RGBL_ERR_INVALID, and every output of every problem stays as the caller left it"""
    case = sized_case(40, 5, seed=31)
    base = tc.problem(case)
    N, n1, n2 = case["N"], len(case["xy1"]), len(case["xy2"])
    fr = resident(lib, np.zeros((n1 + 5, 2), np.float32))
    first = int(case["idx1"][0])

    def broken(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c
    few = np.full(n1, -1, np.int32)
    few[case["idx1"][:7]] = case["idx2"][:7]
    bad = {"sample too large": broken("samples", (2, 1), N),
           "sample negative": broken("samples", (0, 0), -1),
           "sample repeated": broken("samples", (4, 7), base["samples"][4, 0]),
           "seven matches": dict(base, matches12=few, samples=np.tile(np.arange(8, dtype=np.int32) % 7, (5, 1))),
           "match too large": broken("matches12", first, n2),
           "match -2": broken("matches12", first, -2),
           "K NaN": broken("K", 1, np.nan),
           "K inf": broken("K", 2, np.inf),
           "sigma NaN": dict(base, sigma=np.float32(np.nan)),
           "sigma inf": dict(base, sigma=np.float32(np.inf)),
           "n1 too large": dict(base, n1=N_MAX + 1),
           "n2 too large": dict(base, n2=N_MAX + 1),
           "n1 negative": dict(base, n1=-1),
           "n_hyp negative": dict(base, n_hyp=-1),
           "n_hyp too large": dict(base, n_hyp=N_HYP_MAX + 1),
           "no keys 1": dict({k: v for k, v in base.items() if k != "xy1"}, n1=n1),
           "no keys 2": dict({k: v for k, v in base.items() if k != "xy2"}, n2=n2),
           "no matches": dict({k: v for k, v in base.items() if k != "matches12"}, n1=n1),
           "no samples": dict({k: v for k, v in base.items() if k != "samples"}, n_hyp=5),
           "frame of another size": dict({k: v for k, v in base.items() if k != "xy1"}, n1=n1, device1=fr)}
    for what, pr in bad.items():
        for batch in (False, True):
            keep = []
            I, O = (L.TwoViewInput * 2)(), (L.TwoViewOutput * 2)()
            F.ORBmatcher._two_view_input(base, keep, I[0])
            F.ORBmatcher._two_view_input(pr, keep, I[1])
            bufs = []
            for b in range(2):
                C.memset(C.byref(O[b]), 0x5a, C.sizeof(L.TwoViewOutput))
                bufs.append((np.full((n1, 3), 9, np.float32), np.full(n1, 9, np.uint8), np.full((5, 2), 9, np.float32),
                             np.full((5, 18), 9, np.float32), np.full(n1, 9, np.uint8), np.full(n1, 9, np.uint8)))
                O[b].p3d, O[b].triangulated, O[b].scores, O[b].models, O[b].inliers_h, O[b].inliers_f = [a.ctypes.data for a in bufs[b]]
            before = [bytes(O[0]), bytes(O[1])]
            if batch:   # the good problem in front of the bad one: neither is written
                rc = lib.rgbl_two_view_reconstruct_batch(mt.h, 2, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p))
            else:
                rc = lib.rgbl_two_view_reconstruct(mt.h, C.byref(I[1]), C.byref(O[1]))
            assert rc == L.ERR_INVALID, (what, batch, rc)
            assert [bytes(O[0]), bytes(O[1])] == before, (what, batch)
            assert all((a == 9).all() for bb in bufs for a in bb), (what, batch)
            if not batch:   # the host build refuses the same things (and every resident frame)
                assert lib.rgbl_two_view_reconstruct_host(C.byref(I[1]), C.byref(O[1])) == L.ERR_INVALID, what
                assert bytes(O[1]) == before[1] and all((a == 9).all() for a in bufs[1]), what
    assert lib.rgbl_two_view_reconstruct(mt.h, None, None) == L.ERR_INVALID
    keep = []
    I = F.ORBmatcher._two_view_input(base, keep)
    assert lib.rgbl_two_view_reconstruct_host(C.byref(I), None) == L.ERR_INVALID
    fr.close()
    same(mt.TwoViewReconstruct(base), F.two_view_reconstruct_host(base, lib), "after the refused calls")


def check_limits(lib, mt):
    """every size limit from both sides: the highest value is accepted and computed, one past it is refused (check_errors holds
    the refusals of n1, n2 and n_hyp; check_limit_n and check_limit_hyp run their maxima)"""
    case = sized_case(40, 5, seed=33)
    N, n2 = case["N"], len(case["xy2"])
    base = tc.problem(case)

    def set_at(key, idx, value):
        c = dict(base)
        c[key] = np.array(base[key]).copy()
        c[key][idx] = value
        return c
    free2 = int(np.setdiff1d(np.arange(n2), case["idx2"])[-1])
    inside = {"sample N - 1": set_at("samples", (2, 1), N - 1) if N - 1 not in base["samples"][2] else base,
              "eight matches": tc.problem(sized_case(8, 5, seed=34)),
              "match n2 - 1": set_at("matches12", int(case["idx1"][0]), n2 - 1) if n2 - 1 not in case["idx2"] else base,
              "two keys of frame 1 on one of frame 2": set_at("matches12", int(case["idx1"][0]), int(case["idx2"][1])),
              "an unmatched key of frame 2": set_at("matches12", int(case["idx1"][0]), free2)}
    for what, pr in inside.items():
        both(lib, mt, pr, what)
    # n_hyp = 0 is valid whatever N is, and launches nothing
    none = mt.TwoViewReconstruct(dict(base, n_hyp=0, samples=None), fill=FILL)
    assert (none["found"], none["model"], none["exit_code"]) == (0, -1, NO_SCORE)
    keep = []
    O = L.TwoViewOutput()
    I = F.ORBmatcher._two_view_input(dict(base, n_hyp=N_HYP_MAX + 1, samples=np.tile(base["samples"][:1], (N_HYP_MAX + 1, 1))), keep)
    assert lib.rgbl_two_view_reconstruct(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"%d" % N_HYP_MAX in lib.rgbl_last_error()
    # the masks of one call: 2 x n_hyp x ceil(N / 64) words over all problems may not exceed 2^26; 2^20 hypotheses of 65 words
    # are refused before anything is staged
    big = tc.problem(sized_case(64 * 64 + 1, 1, seed=35, extra1=0, extra2=2))
    keep = []
    I = F.ORBmatcher._two_view_input(dict(big, samples=np.tile(big["samples"], (N_HYP_MAX, 1)), n_hyp=N_HYP_MAX), keep)
    assert lib.rgbl_two_view_reconstruct(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"mask words" in lib.rgbl_last_error()
    # the keys of frame 1 of one call: 2^24 over the problems that run; 257 problems of 65535 keys are refused before anything is staged
    wide = tc.problem(sized_case(N_MAX, 1, seed=36, extra1=0, extra2=0))
    keep = []
    I, O = (L.TwoViewInput * 257)(), (L.TwoViewOutput * 257)()
    F.ORBmatcher._two_view_input(wide, keep, I[0])
    for b in range(1, 257):
        C.memmove(C.byref(I[b]), C.byref(I[0]), C.sizeof(L.TwoViewInput))
    assert lib.rgbl_two_view_reconstruct_batch(mt.h, 257, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == L.ERR_INVALID and b"keys of frame 1" in lib.rgbl_last_error()
    assert O[0].model == 0 and O[256].n_inliers == 0
    O = L.TwoViewOutput()
    # n_problems: 32767 problems that run nothing are inside, 32768 are refused
    keep = []
    I, O = (L.TwoViewInput * (B_MAX + 1))(), (L.TwoViewOutput * (B_MAX + 1))()
    F.ORBmatcher._two_view_input(dict(base, n_hyp=0, samples=None), keep, I[0])
    for b in range(1, B_MAX + 1):
        C.memmove(C.byref(I[b]), C.byref(I[0]), C.sizeof(L.TwoViewInput))
    assert lib.rgbl_two_view_reconstruct_batch(mt.h, B_MAX, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == 0
    assert O[B_MAX - 1].model == -1 and O[B_MAX - 1].exit_code == NO_SCORE and O[B_MAX].model == 0
    assert lib.rgbl_two_view_reconstruct_batch(mt.h, B_MAX + 1, C.cast(I, C.c_void_p), C.cast(O, C.c_void_p)) == L.ERR_INVALID


def check_limit_n(lib, mt):
    """two frames of N_MAX keys, every key of frame 1 matched: the first set names matches N_MAX - 1 and 32768"""
    case = sized_case(N_MAX, 2, seed=7, extra1=0, extra2=0, outlier_share=0.0)
    good = [int(g) for g in range(100, 40000, 5000) if g not in (N_MAX - 1, 32768)][:6]
    case["samples"][0] = [N_MAX - 1, 32768] + good
    pr = tc.problem(case)
    assert len(pr["xy1"]) == N_MAX and len(pr["xy2"]) == N_MAX and (pr["matches12"] >= 0).all()
    want = both(lib, mt, pr, "%d matches" % N_MAX)
    assert want["n_inliers"] > 1000
    keep = []
    for key in ("n1", "n2"):
        I, O = F.ORBmatcher._two_view_input(dict(pr, **{key: N_MAX + 1}), keep), L.TwoViewOutput()
        assert lib.rgbl_two_view_reconstruct(mt.h, C.byref(I), C.byref(O)) == L.ERR_INVALID and b"65535" in lib.rgbl_last_error()
    return want["n_inliers"]


def check_limit_hyp(lib, mt, N=20):
    """N_HYP_MAX hypotheses: 64 distinct sets, repeated; the host build computes the 64, every repetition on the device must
    carry the same bits, and the first of the equal maxima wins"""
    case = sized_case(N, 64, seed=11)
    pr64 = tc.problem(case)
    want = F.two_view_reconstruct_host(pr64, lib)
    rep = N_HYP_MAX // 64
    got = mt.TwoViewReconstruct(dict(pr64, samples=np.tile(case["samples"], (rep, 1)), n_hyp=N_HYP_MAX))
    sc = got["scores"].reshape(rep, 64, 2)
    same_bits(sc[0], want["scores"], "the first 64 hypotheses")
    same_bits(sc[-1], want["scores"], "the last 64 hypotheses")
    nan = np.isnan(want["scores"])
    assert (np.isnan(sc) == nan).all() and (sc[:, ~nan] == want["scores"][~nan]).all()
    same_bits(got["models"][-64:], want["models"], "the last 64 models")
    for k in ("best_h", "best_f", "model", "exit_code", "found", "n_inliers"):
        assert got[k] == want[k], (k, got[k], want[k])
    return int(want["n_inliers"])


def check_threads(lib, rounds=4):
    """the call next to other matcher calls from other threads, every thread on a handle of its own"""
    pr = tc.problem(sized_case(257, 20, seed=41))
    want = F.two_view_reconstruct_host(pr, lib)
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
            same(m.TwoViewReconstruct(pr), want, "round %d next to searches" % r)
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
