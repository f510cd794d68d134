"""The library's size limits from both sides on the MI355X (tests/limit_cases.py): everything tests/test_limits_emu.py runs, and
what needs the hardware - real concurrency in the resolve kernels' global-memory form, the three Hamming kernels, the sizes the
emulator is too slow for.  DESIGN.md ("Size limits") has the table."""
import pytest
import torch

import geometry_checks as gc
import limit_cases as lc
import pose_opt_checks as pk
import sim3_checks as sk
import stereo_cases as S
import test_hamming_tracker as ht
from orb_slam3_rgbl_amd import frontend as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SEARCH_NAMES = sorted(gc.SEARCHES)
SQUARE = ("initialization", "search_by_sim3")
OTHER_CAMERA = [("projection", "euroc_undistorted", (12, 1.2)), ("fuse", "small_offset", (16, 1.1)),
                ("projection_sim3_form0", "resized", (8, 1.2))]


# ---- 1. grid searches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_search_in_a_frame_of_65535_features(gpu_lib, name):
    """initialization, search_by_sim3: both frames have 65535 features"""
    lc.check_search_at_limit(gpu_lib, name, n1=lc.N2_MAX if name in SQUARE else 600)


@pytest.mark.parametrize("name,camera,pyramid", OTHER_CAMERA, ids=[c[0] + "-" + c[1] for c in OTHER_CAMERA])
def test_search_in_a_frame_of_65535_features_on_another_camera(gpu_lib, name, camera, pyramid):
    lc.check_search_at_limit(gpu_lib, name, camera, pyramid)


@pytest.mark.parametrize("name", [n for n in SEARCH_NAMES if n not in SQUARE])
def test_search_of_70000_points_in_a_frame_of_65535_features(gpu_lib, name):
    """point indices beyond 16 bits; the greedy searches' resolve kernel in its global-memory form"""
    lc.check_search_at_limit(gpu_lib, name, n1=70000)


@pytest.mark.parametrize("name", lc.POINT_LIMIT_SEARCHES)
def test_search_of_2_to_the_20_minus_1_points(gpu_lib, name):
    lc.check_point_limit(gpu_lib, name)


def test_resident_frame_of_65535_features(gpu_lib):
    lc.check_resident_at_limit(gpu_lib)


def test_grid_searches_refuse_65536_features_and_2_to_the_20_points(gpu_lib):
    lc.check_grid_search_refusals(gpu_lib)


# ---- 2. Hamming scan ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp4", "i8", "0"])
def test_hamming_scan_of_65535_train_rows(gpu_lib, monkeypatch, variant):
    """k_hamming_fp4 (the default), k_hamming_mfma (RGBL_BF_MFMA=i8) and k_hamming_bf (=0), train-set slices on and off, and the
    batch entry point with cap = 65535"""
    if variant == "fp4":
        monkeypatch.delenv("RGBL_BF_MFMA", raising=False)
    else:
        monkeypatch.setenv("RGBL_BF_MFMA", variant)
    ht.check_limit_rows(gpu_lib)
    ht.check_batch_device_at_limit(gpu_lib, DEV)


# ---- 3. stereo ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["right", "left"])
def test_stereo_matches_with_65535_keypoints_in_one_view(gpu_lib, side):
    assert S.case_limit(gpu_lib, DEV, side) > 0


# ---- 4. pose optimisation, 5. Sim3 ---------------------------------------------------------------------------------------------
def test_pose_optimisation_of_65535_features(gpu_lib):
    mt = F.ORBmatcher(0.6, False, lib=gpu_lib)
    pk.check_limit(gpu_lib, mt)
    pk.check_limit_refused(gpu_lib, mt)
    mt.close()


def test_sim3_of_65535_correspondences(gpu_lib):
    mt = F.ORBmatcher(0.6, False, lib=gpu_lib)
    sk.check_limit_n(gpu_lib, mt)
    mt.close()


def test_sim3_of_2_to_the_20_hypotheses(gpu_lib):
    mt = F.ORBmatcher(0.6, False, lib=gpu_lib)
    assert sk.check_limit_hyp(gpu_lib, mt) >= 3
    mt.close()


# ---- 6. ComputeDistinctiveDescriptors and the map refresh ----------------------------------------------------------------------
def test_distinctive_descriptor_of_a_point_at_the_observation_limit(gpu_lib):
    lc.check_distinctive_limit(gpu_lib)
    lc.check_distinctive_refused(gpu_lib)


def test_map_refresh_of_a_point_at_the_observation_limit(gpu_lib):
    lc.check_refresh_limit(gpu_lib)


# ---- 7. SearchByBoW ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1, 2], ids=["kf_f", "kf_two_camera_f", "kf_kf"])
def test_search_by_bow_with_a_bucket_of_16384(gpu_lib, form):
    lc.check_bow_at_limit(gpu_lib, form)


def test_search_by_bow_refuses_a_bucket_of_16385(gpu_lib):
    lc.check_bow_refused(gpu_lib)


# ---- 8. depth module -----------------------------------------------------------------------------------------------------------
def test_depth_of_scans_around_2_to_the_20_points(gpu_lib):
    lc.check_depth_index_limit(gpu_lib)


# ---- 9. extractor, 10. the plain launch grid ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfeatures", [2000, 6000])
def test_extraction_from_an_image_4096_wide(gpu_lib, nfeatures):
    lc.check_extractor_width_limit(gpu_lib, nfeatures)


def test_extractor_refuses_sides_of_4097(gpu_lib):
    lc.check_extractor_side_refused(gpu_lib)


def test_extraction_with_the_longest_node_list(gpu_lib):
    assert lc.check_extractor_node_list_limit(gpu_lib) >= 60000


@pytest.mark.parametrize("batch,xcd_map", [(1, True), (8, True), (8, False)], ids=["one_frame", "batch_of_8", "batch_of_8_RGBL_XCD_MAP_0"])
def test_extraction_with_more_than_65535_detection_cells_in_one_launch(gpu_lib, batch, xcd_map):
    """the slow one: the oracle needs a dozen seconds for each of the two 4096 x 4096 images on 16 levels (computed once)"""
    assert lc.check_extractor_plain_grid(gpu_lib, batch, xcd_map) > 65535


def test_resize_to_more_than_65535_destination_tiles(gpu_lib):
    assert lc.check_resize_plain_grid(gpu_lib) > 65535


# ---- 11. KeyFrameDatabase ------------------------------------------------------------------------------------------------------
def test_kfdb_batch_of_65535_queries(gpu_lib):
    lc.check_kfdb_query_limit(gpu_lib)
