"""One handle, many kinds of call, shuffled.

The test modules share one matcher per module and call it in one fixed order, so a call only ever sees what the same earlier
calls left in the handle's grow-only arena.  A SLAM process calls one handle thousands of times with changing sizes and kinds.
Here the references are computed once (the oracle, or the host build bit for bit), then the calls run on ONE handle in three
fixed-seed permutations, a large and a small size of every family - so that a small call's arrays are carved out of a large
call's leftovers - with host arrays and pool / resident forms mixed and refused calls (one past a limit, a bad index) in
between.  Every result must equal its reference; every refused call must leave its outputs as the caller filled them.

  matcher    a grid search (SearchByProjection), a FeatureVector search (SearchByBoW), the Hamming scan, the Sim3 and MLPnP
             RANSACs, TwoViewReconstruction, pose optimisation, OptimizeSim3, local and global bundle adjustment
  extractor  max_batch 3: noise, a constant image, low contrast, noise again, in batches of 1 / 3 / 2 and with a lapping change
  depth      scans of 0, 64 and max_points points, the map-free (indexed) and the raw path alternating, 0 and 16 keypoints

All sizes are the checks' smallest.  The same tests run on the CPU emulation of the kernel sources and, marked gpu, on the
device; tests/test_alloc_fill.py runs the families with non-zero fresh memory."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O
from orb_slam3_rgbl_amd import _lib as L
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth

SEEDS = (1, 2, 3)
SENTINEL = 0x6B   # what the outputs of a refused call hold before it


class Call:
    """run(mt) -> the result; same(got, want) asserts; want is filled once, before the first permutation"""

    def __init__(self, name, run, same, want=None, reference=None, refused=False):
        self.name, self.run, self.same, self.want, self.reference, self.refused = name, run, same, want, reference, refused


def _arrays_equal(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(g), np.asarray(w)), "result %d differs in %d places" % (k, int((np.asarray(g) != np.asarray(w)).sum()))


# ---- the matcher handle ------------------------------------------------------------------------------------------------------
def matcher_calls(lib, keep):
    """the closures and their references; `keep` receives the pools and resident frames the closures use (closed by the caller)"""
    import gba_checks as gk
    import geometry_checks as gc
    import lba_checks as lk
    import mlpnp_checks as mk
    import parity_checks as pc
    import pose_opt_checks as pk
    import sim3_checks as sk
    import sim3_opt_checks as ok
    import twoview_checks as tk
    calls = []

    # a grid search: SearchByProjection(CurrentFrame, LastFrame), host arrays at the large size, a resident frame at the small one
    def projection(n1, n2, resident):
        s = gc.SEARCHES["projection"]
        case = s.make(gc.camera("small_offset"), (8, 1.2), n1, n2, 500 + n1)
        want, found = s.oracle(case)
        assert found > 0
        if resident:
            f2 = F.DeviceFrame(n2, lib=lib)
            keep.append(f2)
            f2.upload(case["desc2"], case["kp2_xy"], case["kp2_octave"], case.get("uright2"))
            f2.set_grid(case["grid"])
            case = dict(case, device2=f2, **{k: np.zeros_like(case[k]) for k in ("kp2_xy", "kp2_octave", "desc2", "uright2") if k in case})

        def run(mt):
            mt.mfNNratio, mt.mbCheckOrientation = 0.9, True
            return (mt.SearchByProjection(case, 7.0, False)[0],)
        return Call("projection %d x %d%s" % (n1, n2, ", resident frame" if resident else ""), run, _arrays_equal, want)
    calls += [projection(1200, 1000, False), projection(60, 80, True)]

    # a FeatureVector search: SearchByBoW(KeyFrame, Frame)
    def bow(n, nodes):
        kf, fr, *_ = pc.make_triangulation_case(n, seed=700 + n, n_nodes=nodes)
        kf = dict(kf, has_mp=(np.random.default_rng(n).random(n) < 0.7).astype(np.uint8))
        om, onm = O.search_by_bow(kf, fr, 0.7, True)

        def run(mt):
            mt.mfNNratio, mt.mbCheckOrientation = 0.7, True
            m, nm = mt.SearchByBoW(kf, fr)
            return m, np.int64(nm)
        return Call("SearchByBoW %d features, %d nodes" % (n, nodes), run, _arrays_equal, (om, np.int64(onm)))
    calls += [bow(700, 30), bow(40, 5)]

    # the Hamming scan: 2000 train rows in launch slices, and a handful
    def hamming(na, nb):
        a = synth.descriptors(na, 800 + na)
        b, _ = synth.perturbed_descriptors(np.resize(a, (nb, 32)), seed=801 + na)
        return Call("Hamming %d x %d" % (na, nb), lambda mt: mt.BruteForce(a, b), _arrays_equal, O.hamming_bf(a, b))
    calls += [hamming(300, 2000), hamming(5, 33)]

    # Sim3 RANSAC: host arrays large, the pool form small
    big = sk.sized_case(1025, 20, False, seed=5)
    calls.append(Call("sim3 1025 x 20", lambda mt: mt.Sim3Ransac(sk.sc.problem(big), fill=sk.FILL), lambda g, w: sk.same(g, w, "sim3 1025"),
                      F.sim3_ransac_host(sk.sc.problem(big), lib, fill=sk.FILL)))
    small = sk.sized_case(20, 3, True, seed=6)
    pool = F.MapPointPool(256, lib=lib)
    keep.append(pool)
    perm = np.random.default_rng(4).permutation(256).astype(np.int32)
    pool.update(np.concatenate([perm[:20], perm[20:40]]), world_pos=np.concatenate([small["Xw1"], small["Xw2"]]))
    calls.append(Call("sim3 20 x 3, pool form", lambda mt: mt.Sim3Ransac(sk.sc.pool_problem(small, pool, perm[:20], perm[20:40]), fill=sk.FILL),
                      lambda g, w: sk.same(g, w, "sim3 pool"), reference=lambda mt: mt.Sim3Ransac(sk.sc.problem(small), fill=sk.FILL)))

    # MLPnP RANSAC
    for N, h in ((300, 35), (7, 2)):
        pr = mk.mc.problem(mk.sized_case(N, h, seed=7))
        calls.append(Call("mlpnp %d x %d" % (N, h), lambda mt, pr=pr: mt.MLPnPRansac(pr, fill=mk.FILL), lambda g, w, N=N: mk.same(g, w, "mlpnp %d" % N),
                          F.mlpnp_ransac_host(pr, lib, fill=mk.FILL)))
    # TwoViewReconstruction
    for N, h in ((257, 5), (9, 3)):
        pr = tk.tc.problem(tk.sized_case(N, h, seed=8))
        calls.append(Call("two-view %d x %d" % (N, h), lambda mt, pr=pr: mt.TwoViewReconstruct(pr, fill=tk.FILL), lambda g, w, N=N: tk.same(g, w, "two-view %d" % N),
                          F.two_view_reconstruct_host(pr, lib, fill=tk.FILL)))

    # pose optimisation: a resident frame and a pool at the large size, host arrays at the small one
    from orb_slam3_rgbl_amd import cases
    pcase = cases.make_pose_opt_case(500, 320, seed=23)
    n, npts = len(pcase["mp_index"]), len(pcase["world_pos"])
    fr = F.DeviceFrame(n, lib=lib).upload(np.zeros((n, 32), np.uint8), pcase["xy"], pcase["octave"], pcase["uright"])
    ppool = F.MapPointPool(1000, lib=lib)
    keep += [fr, ppool]
    slot = np.random.default_rng(1).permutation(1000)[:npts].astype(np.int32)
    ppool.update(slot, world_pos=pcase["world_pos"])
    res = {k: pcase[k] for k in ("mp_index", "q", "t", "K", "bf", "inv_level_sigma2", "n_levels")}
    calls.append(Call("pose optimisation 320 matched, resident frame and pool", lambda mt: mt.PoseOptimization(dict(res, device=fr, pool=ppool, slot=slot), outlier_fill=7),
                      lambda g, w: pk.same(g, w, "pose 320"), F.pose_optimization_host(pcase, lib, outlier_fill=7)))
    scase = pk.sized_case(10, "mixed", seed=2)
    calls.append(Call("pose optimisation 10 matched", lambda mt: mt.PoseOptimization(scase, outlier_fill=7), lambda g, w: pk.same(g, w, "pose 10"),
                      F.pose_optimization_host(scase, lib, outlier_fill=7)))
    # OptimizeSim3
    for matched, fix in ((2049, False), (10, True)):
        case = ok.sized_case(matched, fix, seed=3)
        calls.append(Call("OptimizeSim3 %d matched" % matched, lambda mt, case=case: mt.OptimizeSim3(case, cleared_fill=ok.FILL),
                          lambda g, w, m=matched: ok.same(g, w, "OptimizeSim3 %d" % m), F.optimize_sim3_host(case, lib, cleared_fill=ok.FILL)))
    # local and global bundle adjustment (same(host, device): the argument order of the modules' own comparison)
    for name, case in (("tile_crossings", lk.tile_crossings()), ("minimal", lk.minimal())):
        calls.append(Call("local BA %s" % name, lambda mt, case=case: mt.LocalBundleAdjustment(case, fill=lk.FILL), lambda g, w, name=name: lk.same(w, g, name),
                          F.local_bundle_adjustment_host(case, lib=lib, fill=lk.FILL)))
    for nA in (gk.PANEL_SIZES[5], 1):
        case = gk.sized(nA)
        calls.append(Call("global BA %d free cameras" % nA, lambda mt, case=case: mt.BundleAdjustment(case, fill=gk.FILL), lambda g, w, nA=nA: gk.same(w, g, "gba %d" % nA),
                          F.bundle_adjustment_host(case, lib=lib, fill=gk.FILL)))

    # ---- refused calls: nothing is launched, the outputs stay as the caller filled them
    def hamming_one_past(mt):
        a = np.zeros((4, 32), np.uint8)
        out = [np.full(4, SENTINEL, np.int32) for _ in range(3)]
        rc = lib.rgbl_hamming_bf(mt.h, L.ptr(a), 4, L.ptr(a), 65536, *[L.ptr(o) for o in out])   # the count is refused before a row is read
        assert rc == L.ERR_INVALID and all((o == SENTINEL).all() for o in out)
    mixed = lk.mixed()
    bad_edge = np.array(mixed["edge_point"], copy=True)
    bad_edge[-1] = 40   # one past the last point
    gcase = gk.mixed()
    bad_cam = np.array(gcase["edge_cam"], copy=True)
    bad_cam[5] = -1
    bad_sim3 = dict(sk.sc.problem(small))
    bad_sim3["samples"] = np.array(bad_sim3["samples"], copy=True)
    bad_sim3["samples"][1, 2] = 20   # one past the last correspondence

    def sim3_bad_sample(mt):
        keepalive = []
        I, Out = F.ORBmatcher._sim3_input(bad_sim3, keepalive), L.Sim3Output()
        C.memset(C.byref(Out), SENTINEL, C.sizeof(L.Sim3Output))
        bufs = (np.full(20, SENTINEL, np.uint8), np.full(3, SENTINEL, np.int32), np.full((3, 16), SENTINEL, np.float32))
        Out.inlier, Out.counts, Out.T12_all = [b.ctypes.data for b in bufs]
        before, held = bytes(Out), [b.tobytes() for b in bufs]
        assert lib.rgbl_sim3_ransac(mt.h, C.byref(I), C.byref(Out)) == L.ERR_INVALID
        assert bytes(Out) == before and [b.tobytes() for b in bufs] == held
    calls += [Call("refused: Hamming scan of 65536 train rows", hamming_one_past, None, refused=True),
              Call("refused: local BA, edge_point one past the points", lambda mt: lk.refused(lib, mt, dict(mixed, edge_point=bad_edge), host=False), None, refused=True),
              Call("refused: global BA, edge_cam -1", lambda mt: gk.refused(lib, mt, dict(gcase, edge_cam=bad_cam), host=False), None, refused=True),
              Call("refused: sim3, a sample one past the correspondences", sim3_bad_sample, None, refused=True)]
    return calls


def run_matcher(lib, seed):
    keep = []
    mt = F.ORBmatcher(0.6, False, lib=lib)
    try:
        calls = matcher_calls(lib, keep)
        assert sum(not c.refused for c in calls) >= 12
        for c in calls:   # a reference that is the library's own host-array form: taken on a handle of its own
            if c.reference is not None:
                ref = F.ORBmatcher(0.6, False, lib=lib)
                c.want = c.reference(ref)
                ref.close()
        for s in SEEDS if seed is None else (seed,):
            for i in np.random.default_rng(s).permutation(len(calls)):
                c = calls[i]
                try:
                    got = c.run(mt)
                    if not c.refused:
                        c.same(got, c.want)
                except AssertionError as e:
                    raise AssertionError("permutation %d, %s: %s" % (s, c.name, e)) from e
    finally:
        mt.close()
        for k in keep:
            k.close()


# ---- the extractor handle ------------------------------------------------------------------------------------------------------
def run_extractor(lib, w=200, h=160):
    ex = F.ORBextractor(300, 1.2, 3, 20, 7, w, h, max_batch=3, lib=lib)
    orc = O.Extractor(300, 1.2, 3, 20, 7)
    rng = np.random.default_rng(11)
    noise_a, noise_b = (rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2))
    flat = np.full((h, w), 77, np.uint8)
    low = (100 + 9 * (rng.random((h, w)) > 0.97)).astype(np.uint8)
    images = {"noise a": noise_a, "constant": flat, "low contrast": low, "noise b": noise_b}
    laps = ((0, 0), (50, 120))
    want = {(k, lap): orc(img, lap) for k, img in images.items() for lap in laps}   # once
    assert len(want[("noise a", (0, 0))][0]) > 100 and len(want[("constant", (0, 0))][0]) == 0
    # noise, then constant, then low contrast, then noise: batches 1 / 3 / 2, the lapping area changes in between
    calls = [(("noise a",), laps[0]), (("constant", "constant", "constant"), laps[0]), (("low contrast", "constant"), laps[0]), (("noise b",), laps[0]),
             (("noise a", "constant", "low contrast"), laps[1]), (("noise b",), laps[1]), (("constant", "noise a"), laps[0]), (("low contrast",), laps[0]),
             None]   # None: the refused call
    cap = ex.max_keypoints

    def refused():
        imgs = np.zeros((4, h, w), np.uint8)
        out = [np.full((4, cap, 7), SENTINEL, np.uint32), np.full((4, cap, 32), SENTINEL, np.uint8), np.full(4, SENTINEL, np.int32), np.full(4, SENTINEL, np.int32)]
        held = [o.tobytes() for o in out]
        rc = lib.rgbl_extract_batch(ex.h, L.ptr(imgs), 4, w, h, w, w * h, 0, 0, L.ptr(out[0]), L.ptr(out[1]), cap, L.ptr(out[2]), L.ptr(out[3]))
        # the extractor's contract for every error return: no keypoint or descriptor is written, the counts read 0 and monoIndex -1
        assert rc == L.ERR_INVALID and [o.tobytes() for o in out[:2]] == held[:2] and (out[2] == 0).all() and (out[3] == -1).all(), "a batch one past max_batch"
    try:
        for s in SEEDS:
            for i in np.random.default_rng(s).permutation(len(calls)):
                if calls[i] is None:
                    refused()
                    continue
                names, lap = calls[i]
                imgs = np.stack([images[k] for k in names])
                res = ex.extract_batch(imgs, lap) if len(names) > 1 else [ex(imgs[0], None, lap)]
                for b, (kps, desc, mono) in enumerate(res):
                    okps, odesc, omono = want[(names[b], lap)]
                    what = "permutation %d, call %s lapping %s, frame %d" % (s, names, lap, b)
                    import parity_checks as pc
                    pc.assert_keypoints_equal(kps, okps, what)
                    assert np.array_equal(desc, odesc) and mono == omono, what
    finally:
        ex.close()


# ---- the depth handle ------------------------------------------------------------------------------------------------------------
def run_depth(lib, w=96, h=64, max_points=300):
    K = np.array([[80, 0, w / 2, 0], [0, 80, h / 2, 0], [0, 0, 1, 0]], np.float32)
    proj = F.projection_matrix(K, np.eye(4, dtype=np.float32), lib)
    dm = F.DepthModule(proj, w, h, max_points=max_points, max_keypoints=16, lib=lib)
    P = O.make_depth_params(proj)
    rng = np.random.default_rng(12)

    def scan(n):
        z = rng.uniform(6, 60, n)
        return np.ascontiguousarray(np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.35, 0.35, n) * z, z, np.ones(n)]).astype(np.float32))
    scans = {n: scan(n) for n in (0, 64, max_points)}
    kps = {0: np.zeros((0, 2), np.float32), 16: np.stack([rng.uniform(1, w - 2, 16), rng.uniform(1, h - 2, 16)], 1).astype(np.float32)}
    want = {(n, k): O.depth(P, scans[n], w, h, kps[k], kps[k][:, 0]) for n in scans for k in kps}   # once
    assert (want[(max_points, 16)][0] > 0).sum() > 3
    # the indexed path (no maps) and the raw path (maps) alternate
    calls = [(n, k, maps) for n in scans for k in kps for maps in (False, True)] + [None]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

    def refused():
        cloud = scan(max_points + 1)
        out = [np.full(16, SENTINEL, np.float32), np.full(16, SENTINEL, np.float32), np.full((h, w), SENTINEL, np.float32), np.full((h, w), SENTINEL, np.float32)]
        before = [o.copy() for o in out]
        rc = lib.rgbl_depth_compute(dm.h, L.ptr(cloud), max_points + 1, max_points + 1, w, h, L.ptr(kps[16]), L.ptr(np.ascontiguousarray(kps[16][:, 0])), 16,
                                    *[L.ptr(o) for o in out])
        assert rc != L.RGBL_OK and all(np.array_equal(bits(o), bits(b)) for o, b in zip(out, before)), "a scan one past max_points"
    try:
        for s in SEEDS:
            order = list(np.random.default_rng(s).permutation(len(calls)))
            for i in order:
                if calls[i] is None:
                    refused()
                    continue
                n, k, maps = calls[i]
                d, ur, raw, proc = want[(n, k)]
                dm.CalculateDepthFromPcd(kps[k], kps[k], scans[n], w, h, want_maps=maps)
                what = "permutation %d: %d points, %d keypoints, %s" % (s, n, k, "maps" if maps else "no maps")
                assert np.array_equal(bits(dm.mvDepth), bits(d)) and np.array_equal(bits(dm.mvuRight), bits(ur)), what
                if maps:
                    assert np.array_equal(bits(dm.RawDepthMap), bits(raw)) and np.array_equal(bits(dm.ProcessedDepthMap), bits(proc)), what
    finally:
        dm.close()


# ---- CPU emulation of the kernel sources ----------------------------------------------------------------------------------------
def test_emu_matcher(emu_lib):
    run_matcher(emu_lib, None)


def test_emu_extractor(emu_lib):
    run_extractor(emu_lib)


def test_emu_depth(emu_lib):
    run_depth(emu_lib)


# ---- the device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_matcher(gpu_lib):
    run_matcher(gpu_lib, None)


@pytest.mark.gpu
def test_gpu_extractor(gpu_lib):
    run_extractor(gpu_lib)


@pytest.mark.gpu
def test_gpu_depth(gpu_lib):
    run_depth(gpu_lib)
