"""No result may depend on what a buffer held before the library wrote it.

Every handle works out of memory it does not clear: the matcher's grow-only arena (37 arrays of a call are hc.scratch<>() and
travel with no upload), the extractor's ~20 buffers of which three are memset, the depth module's generation-tagged index maps,
the FAST counters "left at zero by the quad-tree workgroups", the pyramids' slack bytes.  That is correct only if every kernel
writes an element before it reads it - and a fresh hipMalloc (like the emulator's large posix_memalign) is zero pages, so the
rest of the suite sees zeros.  Here every family of kernels runs in a fresh child process with RGBL_ALLOC_FILL set (csrc/common.h:
every block the library allocates is filled with that byte, every grow-only staging block before each call that reuses it):

  0xFF  reads as -1 (this code's usual "none"), as NaN and as a full counter
  0x5A  reads as a large positive int, as a finite 1.5e16 and as a "true" flag - what a read that happens to see -1 would hide

The children run the suite's own directed checks at their smallest sizes against the references they have everywhere else
(tests/alloc_fill_cases.py).  The emulator tier runs with the CPU suite; the GPU tier (marked gpu) runs the product library, one
child at a time, each under its own time limit - after a child that ends by a signal or at its limit the remaining parameters
fail with "not started after a fault" and start no further GPU process.

test_every_kernel_is_in_the_table is the guard for later work: KERNELS names, for every __global__ of csrc, the check of
alloc_fill_cases.FAMILIES that launches it; a kernel that is added and not entered here fails the test.  (The table was
checked against the launches the emulator saw for each labelled check.)  The two test-only kernels k_selftest_wrappers and
k_test_block_sort are exempt by name.

Mutation check (two scratch copies, emulator tier, both bytes):
  - alloc_scratch (csrc/extractor.hip) without the hipMemset of d_levelcnt.  test_emulator[extractor-0x5a] fails in
    extractor:edge_cases (the constant image comes back with keypoints); with 0xff the child ends by a signal in
    extractor:partial_batches - a counter read as an index; test_filled_memory_under_address_sanitizer reports it in
    k_fast_cells<72, 256, 80> at the program's first extraction.
  - rgbl_search_for_triangulation's `matches12 = hc.put_fill<int32_t>(n1, 0xff)` replaced by hc.scratch<int32_t>(n1).
    test_emulator[feature_vector-0xff] passes - the fill is the very bytes the array starts from, the reason why 0xff alone
    is not enough - and test_emulator[feature_vector-0x5a] fails: the child ends by a signal in feature_vector:bucket_sizes.

CPU wall time (8 CPUs, -n 6, -m "not gpu"): 354 s for the parent commit, 409 s with the additions (WALL_TIME below)."""
import fcntl
import glob
import os
import re
import subprocess
import sys

import pytest

import alloc_fill_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
BUILD = os.path.join(TESTS, "_build")
CSRC = os.path.join(ROOT, "orb_slam3_rgbl_amd", "csrc")
EMU_LIB = os.path.join(BUILD, "librgbl_frontend_emu.so")
GPU_CHILD_LIMIT = 180   # seconds; a family takes a few seconds on the card, most of them in the CPU references
EXEMPT = {"k_selftest_wrappers", "k_test_block_sort"}   # test-only kernels

# kernel -> "family:label" of alloc_fill_cases.FAMILIES: a check that launches it
KERNELS = {
    # extractor (csrc/extractor_kernels.h, octree_labels.h)
    "k_resize_linear": "extractor:edge_cases",
    "k_fast_cells": "extractor:edge_cases",
    "k_gauss7": "extractor_paths:wide_loads",
    "k_octree": "extractor:empty_root",
    "k_orient_brief": "extractor:edge_cases",
    "k_lapping_permute": "extractor:replay",
    "k_compact_cells": "extractor_paths:batch_of_eight",
    "k_octree_moving": "extractor_paths:key_moving_quadtree",
    "k_stereo_match": "stereo:tiles_65_129",
    "k_stereo_filter": "stereo:filter_small",
    "k_cvt_gray": "ingest:cvt_color",
    "k_undistort": "ingest:undistort",
    "k_frame_capture": "feature_vector:device_frames",
    # ingest (resize.hip, rectify.hip, records.hip)
    "k_resize_image": "ingest:resize",
    "k_remap_linear": "ingest:remap",
    "k_remap_gather": "ingest:remap",
    "k_pack_records": "ingest:records",
    "k_pack_records_empty": "ingest:records",
    # depth.hip
    "k_project_index": "depth:partial_batches_generation_wrap",
    "k_project_write": "depth:edge_cases",
    "k_inverse_dilate": "depth:edge_cases",
    "k_average_filter": "depth:three_methods",
    "k_gather_depth": "depth:edge_cases",
    "k_gather_depth_sparse": "depth:sparse",
    "k_nn_depth": "depth:three_methods",
    # matcher.hip: the Hamming scans
    "k_hamming_fp4": "hamming:fp4",
    "k_hamming_merge": "hamming:fp4",
    "k_hamming_mfma": "hamming:i8",
    "k_hamming_bf": "hamming:valu",
    # matcher.hip: the grid searches and the local map
    "k_proj_grid": "grid_searches:projection",
    "k_proj_candidates": "grid_searches:projection",
    "k_proj_resolve": "grid_searches:projection",
    "k_fuse_search": "grid_searches:fuse",
    "k_local_candidates": "grid_searches:local_points",
    "k_local_resolve": "grid_searches:local_points",
    "k_init_candidates": "grid_searches:initialization",
    "k_init_resolve": "grid_searches:initialization",
    "k_frustum": "grid_searches:local_map",
    "k_map_points_scatter": "grid_searches:local_map",
    # matcher.hip: the FeatureVector searches, the vocabulary, the map
    "k_search_by_bow": "feature_vector:bucket_sizes",
    "k_search_by_bow_rig": "feature_vector:bucket_sizes",
    "k_search_triangulation": "feature_vector:bucket_sizes",
    "k_bow_descend": "feature_vector:bow_transform",
    "k_distinctive": "feature_vector:distinctive",
    "k_map_refresh_normal": "map:map_refresh",
    "k_map_refresh_desc": "map:map_refresh",
    "k_new_points": "map:new_points",
    # kfdb.hip
    "k_kfdb_common": "feature_vector:kfdb",
    "k_kfdb_score": "feature_vector:kfdb",
    "k_kfdb_compact": "feature_vector:kfdb",
    # the element-wise device hooks (matcher.hip, optimize.hip): their arrays are allocated per call
    "k_test_logf": "map:device_hooks",
    "k_test_np_cos_parallax": "map:device_hooks",
    "k_test_po_math": "map:device_hooks",
    "k_test_so_exp": "map:device_hooks",
    # ransac.hip
    "k_sim3_hypotheses": "solvers:sim3",
    "k_sim3_select": "solvers:sim3",
    "k_mlpnp_hypotheses": "solvers:mlpnp",
    "k_mlpnp_select": "solvers:mlpnp",
    "k_tv_normalize": "solvers:two_view",
    "k_tv_hypotheses": "solvers:two_view",
    "k_tv_select": "solvers:two_view",
    "k_tv_check_rt": "solvers:two_view",
    "k_tv_decide": "solvers:two_view",
    # optimize.hip
    "k_pose_opt": "solvers:pose_optimisation",
    "k_sim3_opt": "solvers:sim3_optimisation",
    # lba.hip
    "k_lba_gather_points": "bundle_adjustment:lba_pool",
    "k_lba_pool_write": "bundle_adjustment:lba_pool",
    "k_lba_linearise": "bundle_adjustment:lba_minimal",
    "k_lba_point_sums": "bundle_adjustment:lba_minimal",
    "k_lba_cam_blocks": "bundle_adjustment:lba_minimal",
    "k_lba_sums": "bundle_adjustment:lba_minimal",
    "k_lba_trial_edges": "bundle_adjustment:lba_mixed",
    "k_lba_schur": "bundle_adjustment:lba_tile_crossings",
    "k_lba_factor": "bundle_adjustment:lba_mixed",
    "k_lba_trial_points": "bundle_adjustment:lba_mixed",
    "k_lba_flags": "bundle_adjustment:lba_mixed",
    # gba.hip
    "k_gba_schur": "bundle_adjustment:gba_partial_panel",
    "k_gba_diag": "bundle_adjustment:gba_partial_panel",
    "k_gba_start": "bundle_adjustment:gba_partial_panel",
    "k_gba_forward": "bundle_adjustment:gba_partial_panel",
    "k_gba_scale": "bundle_adjustment:gba_partial_panel",
    "k_gba_backward": "bundle_adjustment:gba_partial_panel",
    "k_gba_finish": "bundle_adjustment:gba_partial_panel",
    "k_gba_trailing": "bundle_adjustment:gba_three_panels",
    "k_gba_rows": "bundle_adjustment:gba_failed_pivot_in_a_later_panel",
}

# Wall time of `pytest tests -m "not gpu" -n 6` on one 8-CPU machine: the parent commit (2140 passed), and the same run with this
# file, tests/test_call_order.py and the sanitizer program added (2169 passed): + 55 s, 16 % of the parent's time (the budget is
# a fifth).  The slowest child (extractor, 0xff) takes 27 s there; the two programs under AddressSanitizer share their objects.
WALL_TIME = {"parent_s": 354, "with_additions_s": 409}


def kernels_of_csrc():
    """every __global__ name in csrc/*.hip and csrc/*.h (definitions and prototypes; templates included)"""
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        src = open(path).read()
        for m in re.finditer(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", src):
            names.add(m.group(1))
    return names


def test_every_kernel_is_in_the_table():
    found = kernels_of_csrc()
    assert len(found) > 80 and {"k_fast_cells", "k_gba_rows", "k_lba_schur", "k_octree", "k_resize_image"} <= found, "the expression lost the kernels"
    missing = sorted(found - set(KERNELS) - EXEMPT)
    assert not missing, "kernels without a check under RGBL_ALLOC_FILL (enter them in KERNELS, with a check that launches them): %s" % missing
    gone = sorted(set(KERNELS) - found)
    assert not gone, "KERNELS names kernels csrc no longer has: %s" % gone
    known = ac.labels()
    unknown = sorted({v for v in KERNELS.values() if v not in known})
    assert not unknown, "KERNELS names checks alloc_fill_cases.FAMILIES does not have: %s" % unknown
    idle = sorted(f for f in ac.FAMILIES if not any(v.startswith(f + ":") for v in KERNELS.values()))
    assert not idle, "families no kernel is entered for: %s" % idle


def test_the_switch_is_documented():
    for path in ("README.md", os.path.join("include", "rgbl_frontend.h")):
        assert "RGBL_ALLOC_FILL" in open(os.path.join(ROOT, path)).read(), path


def test_every_allocation_goes_through_the_two_helpers():
    """hipMalloc / hipHostMalloc appear in csrc only inside device_alloc / pinned_alloc of common.h"""
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        src = re.sub(r"//[^\n]*", "", open(path).read())
        calls = re.findall(r"\bhip(?:Host|Ext)?Malloc(?:Managed|Async|Pitch)?\s*\(", src)
        assert len(calls) == (2 if os.path.basename(path) == "common.h" else 0), (path, calls)


def test_filled_memory_under_address_sanitizer():
    """tests/alloc_fill_bounds.cpp: one call each of the extractor, the depth module, the Hamming scan, SearchByProjection, the
    Sim3 RANSAC and the local bundle adjustment per byte, from exactly-sized heap blocks, in a stand-alone program built with
    -fsanitize=address (like tests/wide_loads_bounds.cpp; CPU only): an index read from filled memory is a report here.  The
    two bytes give the same results."""
    import test_wide_loads as wl
    exe = wl.build_bounds_exe("alloc_fill_bounds")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    env.pop("RGBL_ALLOC_FILL", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and "AddressSanitizer" not in res.stderr, res.stdout[-3000:] + res.stderr[-6000:]
    assert "bounds ok" in res.stdout and res.stdout.count("fill ok") == 2
    runs = res.stdout.split("RGBL_ALLOC_FILL=")[1:]
    assert [r.split("\n", 1)[0] for r in runs] == ["0xff", "0x5a"]
    assert runs[0].split("\n", 1)[1].split("fill ok")[0] == runs[1].split("\n", 1)[1].split("fill ok")[0], res.stdout


def run_child(lib_path, family, byte, limit):
    """-> (returncode or None at the limit, output)"""
    env = dict(os.environ, RGBL_ALLOC_FILL="0x%02x" % byte)
    try:
        res = subprocess.run([sys.executable, os.path.join(TESTS, "alloc_fill_cases.py"), lib_path, family], env=env, capture_output=True, text=True,
                             timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        out = (e.stdout or b"").decode("utf-8", "replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        return None, out
    return res.returncode, res.stdout[-4000:] + res.stderr[-6000:]


PARAMS = [(f, b) for f in ac.FAMILIES for b in ac.BYTES]
IDS = ["%s-0x%02x" % p for p in PARAMS]


@pytest.mark.parametrize("family,byte", PARAMS, ids=IDS)
def test_emulator(emu_lib, family, byte):
    rc, out = run_child(EMU_LIB, family, byte, 900)
    assert rc == 0 and "ALLOC_FILL_OK %s %d" % (family, len(ac.FAMILIES[family])) in out, out


_FAULT = []   # what ended by a signal or at its limit in this session (under pytest-xdist: a file per test run, shared by the workers)


def _fault_file():
    uid = os.environ.get("PYTEST_XDIST_TESTRUNUID")
    return os.path.join(BUILD, ".alloc_fill_fault.%s" % uid) if uid else None


def _fault_seen():
    f = _fault_file()
    if f and os.path.exists(f):
        return open(f).read()
    return _FAULT[0] if _FAULT else None


def _fault_note(what):
    _FAULT.append(what)
    if _fault_file():
        with open(_fault_file(), "w") as f:
            f.write(what)


@pytest.mark.gpu
@pytest.mark.parametrize("family,byte", PARAMS, ids=IDS)
def test_mi355x(gpu_lib, family, byte):
    os.makedirs(BUILD, exist_ok=True)
    with open(os.path.join(BUILD, ".alloc_fill_gpu.lock"), "w") as lock:   # one child at a time, whatever runs the tests
        fcntl.flock(lock, fcntl.LOCK_EX)
        if _fault_seen():
            pytest.fail("not started after a fault: %s" % _fault_seen())
        rc, out = run_child("product", family, byte, GPU_CHILD_LIMIT)
        if rc is None or rc < 0 or rc in (124, 134, 137, 139):
            what = "%s with RGBL_ALLOC_FILL=0x%02x %s" % (family, byte, "ran into its limit of %d s" % GPU_CHILD_LIMIT if rc is None else "ended with status %d" % rc)
            _fault_note(what)
            pytest.fail(what + "\n" + out)
    assert rc == 0 and "ALLOC_FILL_OK %s %d" % (family, len(ac.FAMILIES[family])) in out, out
