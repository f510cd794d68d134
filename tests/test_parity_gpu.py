"""Parity tests proper: the HIP path on a real MI355X, called through the C ABI, against the CPU oracle."""
import os

import numpy as np
import pytest

import parity_checks as pc
from orb_slam3_rgbl_amd import frontend as F
from orb_slam3_rgbl_amd import synth

pytestmark = pytest.mark.gpu


def test_extractor_kitti_cfg2_bit_exact(gpu_lib):
    # BASELINE.json configs[1]: KITTI-size frames, nFeatures = 2000, FAST 12/7, bit-exact vs CPU
    n = pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, frames=range(6), stages=False)
    assert n > 6 * 1900


def test_extractor_stages_kitti(gpu_lib):
    pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, frames=(0,), seq=2, stages=True)


def test_extractor_cfg1_nfeatures_1000(gpu_lib):
    pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 1000, frames=(0, 1), seq=3)


def test_extractor_stereo_thresholds(gpu_lib):
    # Examples/Stereo/KITTI00-02.yaml: iniThFAST 20 / minThFAST 7
    pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, frames=(0, 1), ini=20, mn=7, seq=4)


def test_extractor_lapping_area(gpu_lib):
    # the mono constructor passes vLappingArea = {0, 1000} (Frame.cc:401)
    pc.check_extractor(gpu_lib, 752, 480, 1000, frames=(0,), seq=5, lapping=(0, 400))


def test_extractor_batch_equals_single(gpu_lib):
    pc.check_extractor_batch(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, batch=8)


def test_extractor_large_batch_every_frame(gpu_lib):
    # 160 frames x 8 levels: the quad-tree launch switches to its 256-wide workgroups (>= 1024 problems);
    # every frame is compared with the oracle
    pc.check_extractor_batch(gpu_lib, 480, 320, 700, batch=160, seq=9)


def test_extractor_other_shapes(gpu_lib):
    pc.check_extractor(gpu_lib, 752, 480, 1200, frames=(0,), seq=6, stages=True)      # EuRoC
    pc.check_extractor(gpu_lib, 640, 480, 1000, frames=(0,), seq=7, nlevels=5)
    pc.check_extractor(gpu_lib, 1226, 370, 2000, frames=(0,), seq=8)                  # KITTI 04-12


def test_extractor_fast_kernel_instantiations(gpu_lib):
    # 43-px-wide cells: k_fast_cells<48, 128, 64>; 51-px cells on the last level: k_fast_cells<72, 256, 80>
    pc.check_extractor(gpu_lib, 159, 152, 200, frames=(0, 1), nlevels=1, seq=3, stages=True)
    pc.check_extractor(gpu_lib, 640, 480, 600, frames=(0,), seq=4, stages=True)


@pytest.mark.parametrize("bs", ["64", "128"])
def test_extractor_fast_kernel_waves_per_cell(gpu_lib, bs):
    # one wave per detection cell (what batches of 8 and more frames take) and two (single frames), each forced on both
    os.environ["RGBL_FAST_BS"] = bs
    try:
        pc.check_extractor(gpu_lib, 1241, 376, 2000, frames=(0,), seq=5, stages=True)
        pc.check_extractor_batch(gpu_lib, 400, 300, 500, 8)
        pc.check_extractor_low_contrast(gpu_lib)
        pc.check_extractor_dense_corners(gpu_lib)
        pc.check_extractor_threshold_extremes(gpu_lib)
    finally:
        os.environ.pop("RGBL_FAST_BS", None)


def test_extractor_quadtree_round_by_round(gpu_lib):
    # RGBL_OCTREE_HIST=0: the breadth-first phase of the quad-tree kernel as passes over the keys (rounds 1 - 3) instead of on
    # the pyramid of per-cell counts (the default for batches and for 2 048-node problems); RGBL_OCTREE_LDSKEYS=0 makes single
    # frames take the batch instantiation, i.e. the pyramid: both ways of every shape
    for env in ({"RGBL_OCTREE_HIST": "0"}, {"RGBL_OCTREE_LDSKEYS": "0"}, {"RGBL_OCTREE_LDSKEYS": "0", "RGBL_OCTREE_NCAP": "2048"}):
        os.environ.update(env)
        try:
            pc.check_extractor(gpu_lib, 1241, 376, 2000, frames=(0,), seq=5, stages=True)
            pc.check_extractor(gpu_lib, 333, 217, 500, frames=(0,), nlevels=5, seq=4, stages=True)
            pc.check_extractor_batch(gpu_lib, 400, 300, 500, 8)
            pc.check_extractor_empty_root(gpu_lib)
            pc.check_extractor_edge_cases(gpu_lib)
            pc.check_extractor_dense_corners(gpu_lib)
        finally:
            for k in env:
                os.environ.pop(k, None)


@pytest.mark.parametrize("compact", ["1", "0"])
def test_extractor_cell_compaction_kernel(gpu_lib, compact):
    # batches: the FAST cells write their own slots, k_compact_cells builds the level's dense candidate list (one reservation
    # per 256 cells); RGBL_COMPACT=1 forces it for single frames too, =0 keeps the per-cell reservation inside k_fast_cells
    os.environ["RGBL_COMPACT"] = compact
    try:
        pc.check_extractor(gpu_lib, 1241, 376, 2000, frames=(0,), seq=5, stages=True)
        pc.check_extractor_batch(gpu_lib, 400, 300, 500, 8)
        # 106 cell columns of 36 px (the last two of every row are skipped, ORBextractor.cc:810-822), 424 cells on level 0: two groups
        pc.check_extractor(gpu_lib, 3840, 280, 1500, frames=(0,), nlevels=2, seq=12, stages=True)
        pc.check_extractor_low_contrast(gpu_lib)
        pc.check_extractor_dense_corners(gpu_lib)
        pc.check_extractor_empty_root(gpu_lib)
        pc.check_extractor_edge_cases(gpu_lib)
    finally:
        os.environ.pop("RGBL_COMPACT", None)


def test_instruction_wrappers_on_the_hardware(gpu_lib):
    # mul24 / add_flag / lds_dma16: inline asm and builtins that the CPU emulation replaces by plain C
    from orb_slam3_rgbl_amd import _lib as L
    for n, seed in ((1, 1), (63, 2), (64, 3), (1000, 4), (65536 + 17, 5)):
        L.check(gpu_lib, gpu_lib.rgbl_selftest_wrappers(0, n, seed))


def test_extractor_edge_cases(gpu_lib):
    pc.check_extractor_edge_cases(gpu_lib)
    pc.check_extractor_empty_root(gpu_lib)


def test_extractor_cell_slot_candidates(gpu_lib):
    os.environ["RGBL_DENSE"] = "0"
    try:
        pc.check_extractor(gpu_lib, 1241, 376, 2000, frames=(0,), seq=2, stages=True)
        pc.check_extractor_empty_root(gpu_lib)
    finally:
        os.environ.pop("RGBL_DENSE", None)


def test_extractor_4k_cfg5(gpu_lib):
    # BASELINE.json configs[4]: 3840x2160, nFeatures = 8000
    pc.check_extractor(gpu_lib, 3840, 2160, 8000, frames=(0,), seq=9)


@pytest.mark.parametrize("method", [F.UPS_INVERSE_DILATION, F.UPS_AVERAGE_FILTERING, F.UPS_NEAREST_NEIGHBOR_PIXEL])
def test_depth_kitti(gpu_lib, method):
    assert pc.check_depth(gpu_lib, method) > 50


def test_depth_kernels_and_sizes(gpu_lib):
    for kernel in ((F.KERNEL_RECT, 3, 5), (F.KERNEL_CROSS, 5, 5), (F.KERNEL_ELLIPSE, 7, 5), (F.KERNEL_DIAMOND, 9, 9),
                   (F.KERNEL_DIAMOND, 3, 3)):
        pc.check_depth(gpu_lib, F.UPS_INVERSE_DILATION, kernel=kernel, seed=3)
    pc.check_depth(gpu_lib, F.UPS_INVERSE_DILATION, w=3840, h=2160, n_az=4096, seed=4, n_kp=8000)  # cfg 5: 262144 points


def test_depth_edge_cases(gpu_lib):
    pc.check_depth_edge_cases(gpu_lib)


def test_matcher_bf(gpu_lib):
    pc.check_matcher_known_answers(gpu_lib)
    pc.check_matcher_bf(gpu_lib, 2000, 2000)
    pc.check_matcher_bf(gpu_lib, 8000, 8000, seed=5)   # cfg 5
    pc.check_matcher_bf(gpu_lib, 1, 333)
    pc.check_matcher_bf(gpu_lib, 257, 1)
    pc.check_matcher_bf(gpu_lib, 9000, 8800, seed=6)   # three launch slices, a sweep boundary (8192 train rows) inside the third
    pc.check_matcher_bf(gpu_lib, 300, 20000, seed=7)   # 16 slices of 20 stages


def test_search_for_triangulation(gpu_lib):
    pc.check_triangulation(gpu_lib, 2000, seed=11)
    pc.check_triangulation(gpu_lib, 8000, seed=12)
    pc.check_triangulation(gpu_lib, 1500, seed=13, n_nodes=3)   # buckets beyond kTriCap: their tails are read from global memory


def test_hamming_match_of_consecutive_frames_is_symmetric_property(gpu_lib):
    # size-independent property at full size: matching A against A gives the identity with distance 0
    ex = F.ORBextractor(2000, 1.2, 8, 12, 7, synth.KITTI_W, synth.KITTI_H, lib=gpu_lib)
    kps, desc, _ = ex(synth.Sequence(0).frame(0))
    m = F.ORBmatcher(lib=gpu_lib)
    bi, bd, sd = m.BruteForce(desc, desc)
    assert (bd == 0).all()
    # identical descriptors can exist: the first one wins
    first = np.array([np.nonzero((desc == d).all(1))[0][0] for d in desc[:200]])
    assert np.array_equal(bi[:200], first)
    ex.close(); m.close()


def test_compute_stereo_matches(gpu_lib):
    # Frame::ComputeStereoMatches on the resident pyramids of the two extractors
    assert pc.check_stereo_matches(gpu_lib) > 400                       # KITTI stereo thresholds 20/7
    assert pc.check_stereo_matches(gpu_lib, w=752, h=480, nfeatures=1200, seq=31, mb=0.11, mbf=47.9) > 100   # EuRoC-like


def test_ingest_cvtcolor_then_extract(gpu_lib):
    assert pc.check_ingest_color(gpu_lib, synth.KITTI_W, synth.KITTI_H, nfeatures=2000) > 4000
    pc.check_ingest_color_device_batch(gpu_lib)


def test_ingest_kitti_bin_layout(gpu_lib):
    assert pc.check_ingest_kitti_bin(gpu_lib, w=synth.KITTI_W, h=synth.KITTI_H, n_az=1900, n_kp=1500) > 50
    assert pc.check_ingest_kitti_bin(gpu_lib, method=F.UPS_AVERAGE_FILTERING, seed=8) > 10


@pytest.mark.parametrize("seed,motion,th,mono,ori", [(21, "forward", 7.0, False, True), (22, "forward", 15.0, False, True),
                                                     (23, "backward", 7.0, False, True), (24, "none", 30.0, True, False)])
def test_search_by_projection(gpu_lib, seed, motion, th, mono, ori):
    assert pc.check_search_by_projection(gpu_lib, seed, motion, th, mono, ori) > 300


def test_search_by_projection_edge_cases(gpu_lib):
    pc.check_search_by_projection_edge_cases(gpu_lib)
    assert pc.check_search_by_projection(gpu_lib, 27, "forward", 7.0, False, True, n1=7000, n2=8000) > 1000   # 4K-sized frames


@pytest.mark.parametrize("seed,th,orb_dist,ori", [(61, 10.0, 100, True), (62, 3.0, 64, True), (63, 15.0, 100, False), (64, 10.0, 255, True)])
def test_search_by_projection_keyframe(gpu_lib, seed, th, orb_dist, ori):
    assert pc.check_search_by_projection_keyframe(gpu_lib, seed, th, orb_dist, ori) > 150


@pytest.mark.parametrize("seed,th,ratio", [(41, 1.0, 0.8), (42, 3.0, 0.8), (43, 5.0, 0.8), (45, 15.0, 0.7)])
def test_search_local_points(gpu_lib, seed, th, ratio):
    assert pc.check_search_local_points(gpu_lib, seed, th, ratio) > 200


@pytest.mark.parametrize("seed,window,ratio,ori", [(61, 100, 0.9, True), (62, 100, 0.9, False), (63, 30, 0.6, True), (64, 200, 1.0, True),
                                                   (65, 100, 0.9, True)])
def test_search_for_initialization(gpu_lib, seed, window, ratio, ori):
    n1 = 10000 if seed == 65 else 5000          # Tracking builds the initialisation extractor with 5 * nFeatures (Tracking.cc:601)
    assert pc.check_search_for_initialization(gpu_lib, seed, window, ratio, ori, n1=n1) > 600


def test_bow_transform(gpu_lib, tmp_path):
    assert pc.check_bow_transform(gpu_lib, tmp_path, 10, 4, 2, seed=0) > 500
    assert pc.check_bow_transform(gpu_lib, tmp_path, 10, 5, 4, seed=3, n_feat=8000) > 2000   # 111 k nodes


def test_depth_partial_batches(gpu_lib):
    import torch
    pc.check_depth_partial_batches(gpu_lib, torch.device("cuda", 0), w=620, h=188)


@pytest.mark.parametrize("max_gen", [1, 2, 3])
def test_depth_generation_wrap(gpu_lib, max_gen):
    import torch
    pc.check_depth_partial_batches(gpu_lib, torch.device("cuda", 0), w=620, h=188, max_gen=max_gen)


@pytest.mark.parametrize("kernel", [(F.KERNEL_DIAMOND, 5, 7), (F.KERNEL_DIAMOND, 9, 9), (F.KERNEL_RECT, 5, 7), (F.KERNEL_ELLIPSE, 7, 5),
                                    (F.KERNEL_CROSS, 3, 9)])
def test_depth_sparse_upsampling(gpu_lib, kernel):
    """k_gather_depth_sparse against the oracle's dense map sampled at the keypoints (and the dense path through the same handle)"""
    import torch
    pc.check_depth_sparse(gpu_lib, torch.device("cuda", 0), w=620, h=188, kernel=kernel, batch=4, cap=512)


def test_extractor_partial_batches(gpu_lib):
    pc.check_extractor_partial_batches(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000)


def test_extractor_replay(gpu_lib):
    pc.check_extractor_replay(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000)


def test_extractor_under_full_load(gpu_lib):
    pc.check_extractor_under_load(gpu_lib)


@pytest.mark.parametrize("seed,ratio,ori,nodes", [(51, 0.7, True, 100), (52, 0.7, False, 100), (53, 0.9, True, 30), (54, 0.6, True, 1), (55, 0.8, True, 12)])
def test_search_by_bow(gpu_lib, seed, ratio, ori, nodes):
    assert pc.check_search_by_bow(gpu_lib, seed, ratio, ori, n=2000, nodes=nodes) > 100


@pytest.mark.parametrize("seed,ratio,ori,nodes", [(61, 0.7, True, 100), (62, 0.9, False, 30), (63, 0.6, True, 1), (64, 0.8, True, 4), (65, 0.7, True, 12)])
def test_search_by_bow_two_camera_frame(gpu_lib, seed, ratio, ori, nodes):
    """F.Nleft != -1 (ORBmatcher.cc:298-326, 357-386); nodes = 1 / 4: buckets beyond the 256 positions a wave keeps in registers."""
    nm, both = pc.check_search_by_bow_rig(gpu_lib, seed, ratio, ori, n=2000, nodes=nodes)
    assert nm > 100 and both > 20


@pytest.mark.parametrize("seed,ratio,ori,nodes", [(81, 0.75, True, 100), (82, 0.9, False, 30), (84, 0.8, True, 1), (85, 0.8, True, 6)])
def test_search_by_bow_keyframes(gpu_lib, seed, ratio, ori, nodes):
    assert pc.check_search_by_bow_keyframes(gpu_lib, seed, ratio, ori, n=2000, nodes=nodes) > 50


def test_feature_vector_searches_on_bucket_size_edges(gpu_lib):
    pc.check_bucket_sizes(gpu_lib)


@pytest.mark.parametrize("seed,th", [(91, 3.0), (93, 4.0), (94, 1.5)])
def test_fuse_search(gpu_lib, seed, th):
    assert pc.check_fuse_search(gpu_lib, seed, th) > 80


def test_undistort_keypoints(gpu_lib):
    import torch
    pc.check_undistort(gpu_lib, torch.device("cuda", 0))


def test_distinctive_descriptors(gpu_lib):
    assert pc.check_distinctive_descriptors(gpu_lib, 101, 2000) > 1000


@pytest.mark.parametrize("seed,th,form,maxd", [(111, 4.0, 0, 50), (112, 7.5, 1, 100), (113, 3.0, 1, 100)])
def test_project_search(gpu_lib, seed, th, form, maxd):
    assert pc.check_project_search(gpu_lib, seed, th, form, maxd) > 80


@pytest.mark.parametrize("seed,th", [(121, 7.5), (123, 3.0)])
def test_search_by_sim3(gpu_lib, seed, th):
    assert pc.check_search_by_sim3(gpu_lib, seed, th) > 150


@pytest.mark.parametrize("seed,th,form,ratio", [(151, 8, 0, 1.5), (152, 30, 2, 1.0), (153, 3, 0, 2.5)])
def test_search_by_projection_sim3(gpu_lib, seed, th, form, ratio):
    assert pc.check_search_by_projection_sim3(gpu_lib, seed, th, form, ratio) > 80


def test_stereo_fisheye_matches(gpu_lib):
    # SURVEY 8(f) row f4, second half: Frame::ComputeStereoFishEyeMatches' knnMatch(k = 2) + Lowe ratio on the lapping areas
    pc.check_stereo_fisheye_known_answers(gpu_lib)
    assert pc.check_stereo_fisheye_matches(gpu_lib, 2400, 2300, 800, 700) > 500
    pc.check_stereo_fisheye_matches(gpu_lib, 9000, 8800, 100, 300, seed=8)
    pc.check_stereo_fisheye_matches(gpu_lib, 70, 3, 0, 2)
    pc.check_stereo_fisheye_matches(gpu_lib, 50, 40, 50, 10)


# ---- kernels that can be dispatched but are not on the default path ("missing" 1 and 2) -------------------------

def test_extractor_4k_cfg5_batched(gpu_lib):
    # configs[4] in the form bench.py TIMES it (VERDICT r4 missing 1): a batch of 8 4K frames = k_fast_cells (one wave per cell,
    # own slots) -> k_compact_cells -> k_octree<1024, 2048> on the count pyramid, XCD-aware grids, the split pyramid chain
    pc.check_extractor_batch(gpu_lib, 3840, 2160, 8000, batch=8, seq=9)


def test_pipeline_step_4k_cfg5(gpu_lib):
    # ... and the whole timed step at that size: extract + depth on 262 144-point scans + match, every frame vs the oracle
    assert pc.check_pipeline_step(gpu_lib, 3840, 2160, 8000, batch=8, n_az=4096) > 4000


@pytest.mark.parametrize("mode", ["step", "final"])
def test_pipeline_idle_steps_take_part_in_the_gather(gpu_lib, mode):
    pc.check_pipeline_idle_steps(gpu_lib, mode)


def test_pipeline_step_kitti_cfg2(gpu_lib):
    # the headline's step (KITTI size, 2000 features, 121 600-point scans) on 16 distinct frames, every one checked
    assert pc.check_pipeline_step(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, batch=16, n_az=1900, seq=91) > 1500


def test_extractor_initialisation_extractor_uses_the_key_moving_quadtree(gpu_lib):
    # Tracking.cc:601 builds the monocular initialisation extractor with 5 * nFeatures: 10 000 features on KITTI need more than
    # 2048 quad-tree nodes on level 0, i.e. k_octree_moving (node lists in global memory) instead of the label-based kernel
    n = pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 10000, frames=(0, 1), seq=12)
    assert n > 2 * 8000
    pc.check_extractor_batch(gpu_lib, synth.KITTI_W, synth.KITTI_H, 10000, batch=8, seq=13)   # XCD grid + narrow / wide workgroups


def test_extractor_key_moving_quadtree_forced(gpu_lib, monkeypatch):
    # RGBL_OCTREE_NCAP=0: the same kernel on the usual configurations (2000 features), stage by stage
    monkeypatch.setenv("RGBL_OCTREE_NCAP", "0")
    pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, frames=(0, 2), seq=2, stages=True)
    pc.check_extractor(gpu_lib, 752, 480, 1200, frames=(0,), seq=6)
    pc.check_extractor_empty_root(gpu_lib)
    pc.check_extractor_edge_cases(gpu_lib)
    pc.check_extractor_batch(gpu_lib, 480, 320, 700, batch=160, seq=9)        # >= 1024 problems: the 256-wide workgroups
    monkeypatch.setenv("RGBL_OCTREE_NCAP", "2048")
    pc.check_extractor(gpu_lib, synth.KITTI_W, synth.KITTI_H, 2000, frames=(0,), seq=2)   # label-based kernel, 2048-node LDS lists


@pytest.mark.parametrize("variant", ["i8", "0"])
def test_matcher_bf_other_hamming_kernels(gpu_lib, monkeypatch, variant):
    # RGBL_BF_MFMA=i8: k_hamming_mfma (v_mfma_i32_32x32x32_i8); =0: k_hamming_bf (VALU popcount).  Default: k_hamming_fp4.
    monkeypatch.setenv("RGBL_BF_MFMA", variant)
    pc.check_matcher_known_answers(gpu_lib)
    pc.check_matcher_bf(gpu_lib, 2000, 2000)
    pc.check_matcher_bf(gpu_lib, 8000, 8000, seed=5)
    pc.check_matcher_bf(gpu_lib, 1, 333)
    pc.check_matcher_bf(gpu_lib, 257, 1)
    pc.check_matcher_bf(gpu_lib, 9000, 8800, seed=6)    # more than one sweep of 8192 train rows
    pc.check_stereo_fisheye_known_answers(gpu_lib)
    assert pc.check_stereo_fisheye_matches(gpu_lib, 2400, 2300, 800, 700) > 500


def test_pack_records_on_the_device(gpu_lib):
    # k_pack_records (records.hip) against a numpy pack: 68-byte records, frames back to back, offsets, overflow flag
    import ctypes as C

    import torch

    from orb_slam3_rgbl_amd import _lib as L
    from orb_slam3_rgbl_amd.pipeline import RECORD_BYTES, unpack_records
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    for B, cap, first in ((4, 50, 0), (512, 2411, 0), (37, 300, 123), (1, 7, 0)):
        n_h = rng.integers(-3, cap + 20, B).astype(np.int32)          # counts outside [0, cap] are clamped like the readers do
        n_h[0] = cap
        if B > 2:
            n_h[1] = 0
        kp_h = rng.integers(0, 2 ** 32, (B, cap, 7), dtype=np.uint32)
        desc_h = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
        dep_h = rng.integers(0, 2 ** 32, (B, cap), dtype=np.uint32)
        ur_h = rng.integers(0, 2 ** 32, (B, cap), dtype=np.uint32)
        n, kp, desc, dep, ur = (torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in (n_h, kp_h, desc_h, dep_h, ur_h))
        cl = np.clip(n_h, 0, cap)
        total = int(cl.sum())
        out = torch.full(((first + total) * RECORD_BYTES + 64,), 0xEE, dtype=torch.uint8, device=dev)
        off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        ovf = torch.zeros(1, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        L.check(gpu_lib, gpu_lib.rgbl_pack_records_device(C.c_void_p(s.cuda_stream), p(n), p(kp), p(desc), p(dep), p(ur), B, cap, first,
                                                          first + total, p(out), p(off), p(ovf)))
        s.synchronize()
        assert int(ovf.cpu()[0]) == 0
        assert np.array_equal(off.cpu().numpy(), first + np.concatenate([[0], np.cumsum(cl)]))
        o = out.cpu().numpy()
        assert (o[:first * RECORD_BYTES] == 0xEE).all() and (o[(first + total) * RECORD_BYTES:] == 0xEE).all()   # nothing outside its range
        want = np.concatenate([np.concatenate([kp_h[f, :m].view(np.uint8).reshape(m, 28), desc_h[f, :m],
                                               dep_h[f, :m, None].view(np.uint8).reshape(m, 4),
                                               ur_h[f, :m, None].view(np.uint8).reshape(m, 4)], 1) for f, m in enumerate(cl)])
        assert np.array_equal(o[first * RECORD_BYTES:(first + total) * RECORD_BYTES].reshape(total, RECORD_BYTES), want)
        fr = unpack_records(o[first * RECORD_BYTES:], cl)
        assert all(fr[f]["n"] == cl[f] for f in range(B))
        # one record short: the overflow flag goes up and nothing lands behind the buffer's end
        if total > 0:
            small = torch.full(((first + total) * RECORD_BYTES,), 0xEE, dtype=torch.uint8, device=dev)
            L.check(gpu_lib, gpu_lib.rgbl_pack_records_device(C.c_void_p(s.cuda_stream), p(n), p(kp), p(desc), p(dep), p(ur), B, cap, first,
                                                              first + total - 1, p(small), p(off), p(ovf)))
            s.synchronize()
            assert int(ovf.cpu()[0]) == 1
            assert (small.cpu().numpy()[(first + total - 1) * RECORD_BYTES:] == 0xEE).all()
    # an empty batch leaves its one offset
    off = torch.full((1,), -1, dtype=torch.int64, device=dev)
    L.check(gpu_lib, gpu_lib.rgbl_pack_records_device(None, p(n), p(kp), p(desc), p(dep), p(ur), 0, cap, 5, 5, p(out), p(off), p(ovf)))
    torch.cuda.synchronize(dev)
    assert int(off.cpu()[0]) == 5


@pytest.mark.parametrize("mode", ["step", "final"])
def test_gather_choreography_with_one_rank(gpu_lib, mode):
    # FrontEndPipeline with gather = step | final at world == 1: the pack on the communication stream, the counts through
    # page-locked memory behind an event, the root's device copy and the comm_done / depth_done / match_done events all
    # execute on the hardware (no peer, so no RCCL transfer); the records must decode to the step's own outputs
    pc.check_pipeline_gather(gpu_lib, mode)


def test_pipeline_with_sparse_upsampling(gpu_lib):
    # the batched step without the dense ProcessedDepthMap (rgbl_depth_set_sparse): records equal to the oracle's
    pc.check_pipeline_gather(gpu_lib, "step", sparse_depth=True)


def test_overlapped_frame_hooks(gpu_lib):
    # rgbl_extract_begin + rgbl_depth_prefetch: upload and maps of the scan run next to the extraction of the frame
    pc.check_overlapped_frame(gpu_lib)


def test_extractor_second_fast_pass(gpu_lib):
    # low-contrast frames: the cells that find nothing at iniThFAST run the pre-screen / score / NMS again at minThFAST
    assert pc.check_extractor_low_contrast(gpu_lib, 1241, 376, 20, 7, 0.15, nfeatures=2000, nlevels=8) > 1000
    pc.check_extractor_low_contrast(gpu_lib, 793, 286, 30, 10, 0.08)
    pc.check_extractor_low_contrast(gpu_lib, 1145, 290, 30, 3, 0.15)


def test_prioritised_streams_carry_work(gpu_lib):
    # rgbl_stream_create: a handle works on a lowest- / highest-priority stream exactly as on its own
    import ctypes as C
    from orb_slam3_rgbl_amd import _lib as L
    for prio in (-1, 0, 1):
        st = C.c_void_p()
        L.check(gpu_lib, gpu_lib.rgbl_stream_create(C.byref(st), prio))
        m = F.ORBmatcher(0.6, False, lib=gpu_lib)
        L.check(gpu_lib, gpu_lib.rgbl_matcher_set_stream(m.h, st))
        rng = np.random.default_rng(prio + 5)
        a, b = rng.integers(0, 256, (300, 32), dtype=np.uint8), rng.integers(0, 256, (280, 32), dtype=np.uint8)
        bi, bd, sd = m.BruteForce(a, b)
        d = np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2)
        assert np.array_equal(bd, d.min(1)) and np.array_equal(bi, np.where(d == d.min(1)[:, None], np.arange(280)[None, :], 1 << 30).min(1))
        m.close()
        gpu_lib.rgbl_stream_destroy(st)


@pytest.mark.gpu
def test_device_resident_frames(gpu_lib):
    """rgbl_device_frame on the MI355X: upload / capture (extractor + depth handles -> frame, device to device, with and without
    Frame::UndistortKeyPoints) / FeatureVector, and every matcher entry point that takes a resident frame == the host-array
    call == the oracle."""
    assert pc.check_device_frames(gpu_lib, n=2000, nfeatures=2000, w=1241, h=376)


def test_projection_searches_beyond_the_lds_resolve(gpu_lib):
    """Frames / point sets above kResolveLdsN2 / kResolveLdsN1 take the resolve kernels' global-memory form; a call whose candidate
    lists exceed kResolveLdsList entries (25 640 here, many points beyond kProjCand as well) reads them where the candidate kernel left them."""
    assert pc.check_search_local_points(gpu_lib, 49, 6.0, 0.8, n1=6000, n2=3000) > 1000
    assert pc.check_search_by_projection(gpu_lib, 27, "forward", 15.0, False, True, n1=2500, n2=8300) > 300
    assert pc.check_search_local_points(gpu_lib, 48, 3.0, 0.8, n1=13000, n2=3000) > 300
    assert pc.check_search_for_initialization(gpu_lib, 66, 100, 0.9, True, n1=6500) > 300   # both frames beyond kResolveLdsN2


def test_every_tuning_switch_is_bit_identical(gpu_lib):
    """include/rgbl_frontend.h: 'results are bit-identical under all of them' - batch + single-frame extraction and the Hamming
    scan under every switch that changes a launch path, and the batch path with profiling on."""
    assert pc.check_switches(gpu_lib, w=1241, h=376, nfeatures=2000, batch=8) == 14


def test_bow_transform_on_a_vocabulary_of_orbvoc_size(gpu_lib):
    """Row f4 at the size of the real ORBvoc.txt (k = 10, L = 6: ~10^6 nodes, 30 MB of node descriptors resident in HBM; the file
    itself is not in the image): transform(features, BowVector, FeatureVector, levelsup = 4) of 2000 descriptors from host arrays
    and from a resident frame against the oracle's descent."""
    import time
    t0 = time.time()
    voc = synth.make_vocabulary(10, 6, 11)
    varr = synth.vocabulary_arrays(voc)
    assert varr["n_nodes"] > 800000, varr["n_nodes"]
    rng = np.random.default_rng(3)
    leaves = voc["desc"][voc["is_leaf"] > 0]
    pick = leaves[rng.integers(0, len(leaves), 1500)]
    desc = np.ascontiguousarray(np.concatenate([pick ^ np.packbits(rng.random((len(pick), 256)) < 0.03, axis=1, bitorder="little"),
                                                synth.descriptors(500, 5)]))
    want = pc.O.bow_transform(varr, desc, 4)
    V = F.ORBVocabulary(lib=gpu_lib).from_arrays(varr)
    fr = F.DeviceFrame(len(desc), lib=gpu_lib).upload(desc, np.zeros((len(desc), 2), np.float32), np.zeros(len(desc), np.int32))
    for got in (V.transform(desc, 4), V.prepare_transform_frame(fr, 4)()):
        for g, w, name in zip(got, want, ("word ids", "word values", "node ids", "node offsets", "feature indices")):
            assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), name
    assert len(want[2]) <= 100 and len(want[0]) > 1000   # levelsup = 4 of 6 levels: FeatureVector nodes of tree level 2
    fr.close()
    V.close()
    print("ORBvoc-size vocabulary: %d nodes, %.1f s" % (varr["n_nodes"], time.time() - t0))
