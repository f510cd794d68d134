"""What a child process of tests/test_alloc_fill.py runs: the suite's directed checks at their smallest sizes, grouped into
families, each against the reference it has everywhere else (the oracle, a restatement, or the host build bit for bit).  The
process was started with RGBL_ALLOC_FILL set, so every block the library allocates - and every grow-only staging block a call
reuses - holds that byte and not a fresh page's zeros; the checks do not know.

FAMILIES maps a family to its (label, check) list; a check takes the context `c` (c.lib, c.dev: a torch device, c.devn: None
under the emulator - its device pointers are host pointers -, c.gpu, c.tmp).  tests/test_alloc_fill.py's KERNELS names, for every
kernel of csrc, the "family:label" that launches it."""
import contextlib
import ctypes as C
import os
import sys
import tempfile
import time
import traceback

import numpy as np


@contextlib.contextmanager
def env(**kw):
    """switches that a handle reads when it is created, for the checks inside"""
    saved = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Ctx:
    def __init__(self, lib_path):
        try:
            import torch   # before the library: tests/conftest.py says why
        except ImportError:
            torch = None
        from orb_slam3_rgbl_amd import _lib
        self.gpu = lib_path == "product"
        self.lib = _lib.load() if self.gpu else _lib.bind(lib_path)
        self.dev = torch.device("cuda", 0) if self.gpu else torch.device("cpu")
        self.devn = self.dev if self.gpu else None
        self.tmp = tempfile.mkdtemp(prefix="alloc_fill_")
        self._mt = None

    @property
    def mt(self):
        """one matcher handle per process: the solvers and optimisers carve the same arena one after the other"""
        if self._mt is None:
            from orb_slam3_rgbl_amd import frontend as F
            self._mt = F.ORBmatcher(0.6, False, lib=self.lib)
        return self._mt


def _pc():
    import parity_checks
    return parity_checks


def _F():
    from orb_slam3_rgbl_amd import frontend
    return frontend


# ---- extractor ---------------------------------------------------------------------------------------------------------------------
def _wide_loads(c):
    import test_wide_loads as wl
    wl.check_one_level(c.lib, 0)


def _key_moving(c):
    with env(RGBL_OCTREE_NCAP="0"):
        _pc().check_extractor(c.lib, 333, 217, 500, frames=(0, 1), nlevels=5, seq=4, stages=True)
        _pc().check_extractor_empty_root(c.lib)


def _cell_slots(c):
    with env(RGBL_DENSE="0"):
        _pc().check_extractor(c.lib, 333, 217, 500, frames=(0, 1), nlevels=5, seq=4, stages=True)


def _compact_single(c):
    with env(RGBL_COMPACT="1", RGBL_FAST_BS="64"):
        _pc().check_extractor(c.lib, 333, 217, 500, frames=(0, 1), nlevels=5, seq=4, stages=True)


def _batch_of_eight(c):
    _pc().check_extractor_batch(c.lib, 400, 300, 500, 8)


EXTRACTOR = [
    ("edge_cases", lambda c: _pc().check_extractor_edge_cases(c.lib)),
    ("partial_batches", lambda c: _pc().check_extractor_partial_batches(c.lib, 360, 280, 400)),
    ("replay", lambda c: _pc().check_extractor_replay(c.lib, 360, 280, 400)),
    ("empty_root", lambda c: _pc().check_extractor_empty_root(c.lib)),
    ("low_contrast", lambda c: _pc().check_extractor_low_contrast(c.lib, 300, 220, 30, 10, 0.08, nfeatures=300, nlevels=3)),
]
# the launch paths a switch or the batch size selects
EXTRACTOR_PATHS = [
    ("wide_loads", _wide_loads),
    ("key_moving_quadtree", _key_moving),
    ("cell_slots", _cell_slots),
    ("compact_single_frame", _compact_single),
    ("batch_of_eight", _batch_of_eight),
]


# ---- ingest: colour conversion, undistortion, resize, remap, the feeder, records ------------------------------------------------------
def _resize(c):
    import resize_cases as RC
    for name in ("euroc", "quarter", "up"):
        RC.check_host_case(c.lib, RC.CASES[name][0], 3 if name == "up" else 1)
    RC.check_batch_case(c.lib, c.devn, 3, 2)
    RC.check_extract_resized(c.lib, 200, 160, 160, 128, 1)


def _remap(c):
    import remap_cases as RC
    RC.check_host_case(c.lib, "mixed", 1)
    RC.check_host_case(c.lib, "wild", 3)
    RC.check_batch_case(c.lib, c.devn, "mixed", 1, 2)
    RC.check_extract_rectified(c.lib, 160, 128, 3)


def _varlen(c):
    import feed_cases as fc
    F = _F()
    for method in (F.UPS_INVERSE_DILATION, F.UPS_AVERAGE_FILTERING, F.UPS_NEAREST_NEIGHBOR_PIXEL):
        fc.varlen_batch(c.lib, c.gpu, 160, 96, method, [1025, 0, 255, 1])
    fc.varlen_batch(c.lib, c.gpu, 160, 96, F.UPS_INVERSE_DILATION, [700, 0, 256], sparse=True, seed=3)


def _feeder(c):
    import feed_cases as fc
    fc.feeder_vs_single(c.lib, 320, 200, 300, 4, 3, 1, [[1200, 0, 700], [900, 1]], max_points=1500, slots=2)
    K = (718.856 * 320 / 1241, 718.856 * 320 / 1241, 160.0, 100.0)
    fc.feeder_vs_single(c.lib, 320, 200, 300, 4, 1, 0, [[1000, 800]], max_points=1200, slots=2, K=K, dist=(-0.28, 0.07, 0.0002, 0.00002, 0.0))


def _records(c):
    """k_pack_records against a numpy pack (tests/test_distributed.py's round trip, on this context's device)"""
    import torch

    from orb_slam3_rgbl_amd import _lib as L
    from orb_slam3_rgbl_amd.pipeline import RECORD_BYTES, unpack_records
    rng = np.random.default_rng(0)
    B, cap = 4, 50
    up = lambda a: torch.from_numpy(a).to(c.dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    n = np.array([50, 0, 17, 3], np.int32)
    kp, desc = rng.standard_normal((B, cap, 7)).astype(np.float32), rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    dep, ur = rng.standard_normal((B, cap)).astype(np.float32), rng.standard_normal((B, cap)).astype(np.float32)
    d_n, d_kp, d_desc, d_dep, d_ur = up(n), up(kp), up(desc), up(dep), up(ur)
    out, off, ovf = up(np.zeros(B * cap * RECORD_BYTES, np.uint8)), up(np.zeros(B + 1, np.int64)), up(np.zeros(1, np.int32))
    L.check(c.lib, c.lib.rgbl_pack_records_device(None, p(d_n), p(d_kp), p(d_desc), p(d_dep), p(d_ur), B, cap, 0, B * cap, p(out), p(off), p(ovf)))
    if c.gpu:
        torch.cuda.synchronize()
    assert off.cpu().tolist() == [0, 50, 50, 67, 70] and int(ovf.cpu()[0]) == 0
    fr = unpack_records(out.cpu().numpy(), n)
    for i in range(B):
        m = int(n[i])
        assert fr[i]["n"] == m and np.array_equal(fr[i]["desc"], desc[i, :m])
        assert np.array_equal(fr[i]["kp"], kp[i, :m].view(np.uint8).reshape(m, 28))
        assert np.array_equal(fr[i]["depth"], dep[i, :m]) and np.array_equal(fr[i]["uright"], ur[i, :m])
    L.check(c.lib, c.lib.rgbl_pack_records_device(None, p(d_n), p(d_kp), p(d_desc), p(d_dep), p(d_ur), 0, cap, 5, 5, p(out), p(off), p(ovf)))
    if c.gpu:
        torch.cuda.synchronize()
    assert int(off.cpu()[0]) == 5   # no frame: k_pack_records_empty writes the first offset


INGEST = [
    ("cvt_color", lambda c: _pc().check_ingest_color(c.lib, 340, 256)),
    ("undistort", lambda c: _pc().check_undistort(c.lib, c.devn)),
    ("resize", _resize),
    ("remap", _remap),
    ("varlen_scans", _varlen),
    ("feeder", _feeder),
    ("records", _records),
]


# ---- depth ---------------------------------------------------------------------------------------------------------------------------
def _depth_methods(c):
    F = _F()
    for method in (F.UPS_INVERSE_DILATION, F.UPS_AVERAGE_FILTERING, F.UPS_NEAREST_NEIGHBOR_PIXEL):
        _pc().check_depth(c.lib, method, w=310, h=94, n_az=900, n_kp=200)


DEPTH = [
    ("edge_cases", lambda c: _pc().check_depth_edge_cases(c.lib)),
    ("partial_batches_generation_wrap", lambda c: _pc().check_depth_partial_batches(c.lib, c.devn, max_gen=2)),
    ("sparse", lambda c: _pc().check_depth_sparse(c.lib, c.devn)),
    ("three_methods", _depth_methods),
]


# ---- stereo ---------------------------------------------------------------------------------------------------------------------------
def _stereo(name, *args):
    def run(c):
        import stereo_cases as S
        getattr(S, name)(c.lib, c.dev, *args)
    return run


def _stereo_names(name, table):
    def run(c):
        import stereo_cases as S
        for key in sorted(getattr(S, table)):
            if getattr(S, table)[key][0] < 2048 if table == "TIES" else True:
                getattr(S, name)(c.lib, c.dev, key)
    return run


STEREO = [
    ("tiles_12_33", _stereo("case_tiles", 12, 33)),
    ("tiles_65_129", _stereo("case_tiles", 65, 129)),
    ("ties", _stereo_names("case_ties", "TIES")),
    ("flush_16", _stereo("case_flush", 16)),
    ("flush_17", _stereo("case_flush", 17)),
    ("gate_rows", _stereo("case_gate_rows")),
    ("gate_octaves", _stereo("case_gate_octaves")),
    ("gate_u", _stereo("case_gate_u")),
    ("gate_distance", _stereo("case_gate_distance")),
    ("sad_right_border", _stereo("case_sad_right_border")),
    ("sad_left_border", _stereo("case_sad_left_border")),
    ("sad_rows", _stereo("case_sad_rows")),
    ("sad_bestinc", _stereo("case_sad_bestinc")),
    ("zero_disparity", _stereo("case_zero_disparity")),
    ("filter_small", _stereo_names("case_filter_small", "FILTER_SMALL")),
    ("host_sizes", _stereo("case_host_sizes")),
    ("batch_3", _stereo("case_batch", 3)),
]


# ---- Hamming scan ---------------------------------------------------------------------------------------------------------------------
def _hamming(switch):
    def run(c):
        import test_hamming_tracker as ht
        # 64-row stages, a launch slice per four: 448 rows are 7 stages in one slice, 449 and 513 rows two slices (k_hamming_merge)
        with env(**({"RGBL_BF_MFMA": switch} if switch else {})):
            for nb in (448, 449, 513):
                _pc().check_matcher_bf(c.lib, 130, nb, seed=8)
            _pc().check_matcher_bf(c.lib, 1, 33)
            ht.check_batch_device(c.lib, c.dev)
    return run


HAMMING = [("fp4", _hamming(None)), ("i8", _hamming("i8")), ("valu", _hamming("0")),
           ("fisheye", lambda c: _pc().check_stereo_fisheye_matches(c.lib, 400, 380, 120, 100))]


# ---- grid searches --------------------------------------------------------------------------------------------------------------------
def _search(name):
    def run(c):
        import geometry_checks as gc
        gc.check_search(c.lib, name, "small_offset", (8, 1.2), 300, 400)
    return run


def _search_names():
    import geometry_checks as gc
    return sorted(gc.SEARCHES)


SEARCH_NAMES = ("fuse", "initialization", "local_points", "project_search_form0", "project_search_form1", "projection", "projection_keyframe",
                "projection_mono_wide", "projection_sim3_form0", "projection_sim3_form2", "search_by_sim3")


def _local_map(c):
    import local_map_checks as lc
    lc.check_cull_sizes(c.lib, sizes=(0, 1, 65))
    lc.check_fused(c.lib)
    lc.check_pool(c.lib)


GRID = [(name, _search(name)) for name in SEARCH_NAMES] + [
    ("grid_bounds", lambda c: _pc().check_grid_search_bounds(c.lib)),
    ("local_map", _local_map),
]


# ---- FeatureVector searches, the vocabulary, resident frames, the key-frame database ---------------------------------------------------
def _kfdb(c):
    import kfdb_checks as kc
    kc.check_query_sizes(c.lib, sizes=(1, 63, 300), places=(0, 1))
    kc.check_compaction(c.lib)
    kc.check_arena_growth(c.lib)
    kc.check_batch(c.lib, n=70, Q=3)


FEATURE_VECTOR = [
    ("bucket_sizes", lambda c: _pc().check_bucket_sizes(c.lib)),
    ("triangulation", lambda c: _pc().check_triangulation(c.lib, 600, seed=11)),
    ("bow_transform", lambda c: _pc().check_bow_transform(c.lib, c.tmp, 10, 3, 2, seed=1, n_feat=600)),
    ("distinctive", lambda c: _pc().check_distinctive_descriptors(c.lib, 101, 150)),
    ("device_frames", lambda c: _pc().check_device_frames(c.lib, n=500, nfeatures=400, w=400, h=300)),
    ("kfdb", _kfdb),
]


# ---- the map: refresh, new points ---------------------------------------------------------------------------------------------------------
def _map_refresh(c):
    import map_refresh_checks as mr
    mr.check_sizes(c.lib, 2, points=(1, 65), counts=(0, 1, 65, mr.LDS_ROWS + 1))
    mr.check_rules(c.lib)


def _new_points(c):
    import new_points_checks as nc
    nc.check_sizes(c.lib, 2, sizes=(1, 65, 257))
    nc.check_header_level(c.lib)


def _device_hooks(c):
    """the element-wise device hooks allocate their arrays per call: the device builds of the scalar functions against the host's"""
    import pose_opt_checks as pk
    import sim3_opt_checks as ok
    import test_local_map_gpu as tlm
    import test_new_points_gpu as tnp
    pk.check_math_device(c.lib)
    ok.check_math_device(c.lib)
    tlm.test_device_logf_equals_libm(c.lib)
    tnp.test_stereo_parallax_cosine_device_equals_host(c.lib)


MAP = [("map_refresh", _map_refresh), ("new_points", _new_points), ("device_hooks", _device_hooks)]


# ---- the solvers and optimisers: ONE matcher handle, so each call carves what the last one left -------------------------------------------
def _sim3(c):
    import sim3_checks as sk
    sk.check_size(c.lib, c.mt, sk.NS[0], sk.NHYPS[0], 0)
    sk.check_size(c.lib, c.mt, 65, 5, 1)
    sk.check_degenerate(c.lib, c.mt)


def _mlpnp(c):
    import mlpnp_checks as mk
    mk.check_size(c.lib, c.mt, mk.NS[0], mk.NHYPS[0])
    mk.check_size(c.lib, c.mt, 65, 2)
    mk.check_degenerate(c.lib, c.mt)


def _twoview(c):
    import twoview_checks as tk
    tk.check_size(c.lib, c.mt, tk.NS[0], tk.NHYPS[0])
    tk.check_size(c.lib, c.mt, 65, 3)
    tk.check_degenerate(c.lib, c.mt)


def _pose_opt(c):
    import pose_opt_checks as pk
    for matched in (0, 2, 10, 257):
        pk.check_size(c.lib, c.mt, matched, "mixed")
    pk.check_degenerate_depth(c.lib, c.mt)
    pk.check_all_outliers(c.lib, c.mt)


def _sim3_opt(c):
    import sim3_opt_checks as ok
    for matched in (0, 9, 10, 257):
        ok.check_size(c.lib, c.mt, matched, matched == 10)
    ok.check_degenerate_depth(c.lib, c.mt)
    ok.check_no_edge(c.lib, c.mt)


SOLVERS = [("sim3", _sim3), ("mlpnp", _mlpnp), ("two_view", _twoview), ("pose_optimisation", _pose_opt), ("sim3_optimisation", _sim3_opt)]


def _lba(name):
    def run(c):
        import lba_checks as lk
        lk.check_directed(c.lib, c.mt, name)
    return run


def _lba_pool(c):
    import lba_checks as lk
    lk.check_pool(c.lib, c.mt)


def _gba(name):
    def run(c):
        import gba_checks as gk
        gk.check_directed(c.lib, c.mt, name() if callable(name) else name)
    return run


def _gba_panel(k):
    def name():
        import gba_checks as gk
        return "panel_%d" % gk.PANEL_SIZES[k]
    return name


def _gba_pool(c):
    import gba_checks as gk
    gk.check_pool(c.lib, c.mt)


BUNDLE_ADJUSTMENT = [
    ("lba_minimal", _lba("minimal")), ("lba_mixed", _lba("mixed")), ("lba_tile_crossings", _lba("tile_crossings")),
    ("lba_nan_observation", _lba("nan_observation")), ("lba_pool", _lba_pool),
    ("gba_partial_panel", _gba(_gba_panel(0))), ("gba_three_panels", _gba(_gba_panel(5))),
    ("gba_failed_pivot_in_a_later_panel", _gba("failed_pivot_in_a_later_panel")), ("gba_pool", _gba_pool),
]

FAMILIES = {
    "extractor": EXTRACTOR, "extractor_paths": EXTRACTOR_PATHS, "ingest": INGEST, "depth": DEPTH, "stereo": STEREO, "hamming": HAMMING, "grid_searches": GRID,
    "feature_vector": FEATURE_VECTOR, "map": MAP, "solvers": SOLVERS, "bundle_adjustment": BUNDLE_ADJUSTMENT,
}
BYTES = (0xFF, 0x5A)


def labels():
    return {"%s:%s" % (fam, label) for fam, checks in FAMILIES.items() for label, _ in checks}


def run(lib_path, family, only=None):
    """The child process: every check of `family` (or the one labelled `only`), stopping at the first that fails.  Prints one
    line per check with its wall time and ALLOC_FILL_OK <family> <checks run> at the end."""
    c = Ctx(lib_path)
    c.lib.rgbl_test_alloc_fill.restype = C.c_int
    want = os.environ.get("RGBL_ALLOC_FILL")
    if want is not None:   # the switch is live in this process: the library parsed what the parent set
        F = _F()
        F.ORBmatcher(0.6, False, lib=c.lib).close()
        assert c.lib.rgbl_test_alloc_fill() == int(want, 0), "the library cached %d for RGBL_ALLOC_FILL=%s" % (c.lib.rgbl_test_alloc_fill(), want)
    done = 0
    for label, check in FAMILIES[family]:
        if only and label != only:
            continue
        t0 = time.perf_counter()
        try:
            check(c)
        except BaseException:
            traceback.print_exc()
            print("ALLOC_FILL_FAILED %s:%s with RGBL_ALLOC_FILL=%s" % (family, label, want), flush=True)
            return 1
        print("ok %s:%s %.2f s" % (family, label, time.perf_counter() - t0), flush=True)
        done += 1
    if c._mt is not None:
        c._mt.close()
    print("ALLOC_FILL_OK %s %d" % (family, done), flush=True)
    return 0


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    sys.exit(run(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None))
