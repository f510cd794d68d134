"""The library's size limits from both sides, kernel sources under the SIMT emulator: the cases of tests/limit_cases.py that the
emulator runs in seconds.  The larger ones (and everything that needs real concurrency or the hardware's grid) are in
tests/test_limits_gpu.py; DESIGN.md ("Size limits") says which limit is tested where."""
import pytest

import geometry_checks as gc
import limit_cases as lc

SEARCH_NAMES = sorted(gc.SEARCHES)
SQUARE = ("initialization", "search_by_sim3")      # n1 = n2: 65535 x 65535 is the GPU tier's
OTHER_CAMERA = [("projection", "euroc_undistorted", (12, 1.2)), ("fuse", "small_offset", (16, 1.1)),
                ("projection_sim3_form0", "resized", (8, 1.2))]


@pytest.mark.parametrize("name", [n for n in SEARCH_NAMES if n not in SQUARE])
def test_search_in_a_frame_of_65535_features(emu_lib, name):
    lc.check_search_at_limit(emu_lib, name)


@pytest.mark.parametrize("name,camera,pyramid", OTHER_CAMERA, ids=[c[0] + "-" + c[1] for c in OTHER_CAMERA])
def test_search_in_a_frame_of_65535_features_on_another_camera(emu_lib, name, camera, pyramid):
    lc.check_search_at_limit(emu_lib, name, camera, pyramid)


def test_grid_searches_refuse_65536_features_and_2_to_the_20_points(emu_lib):
    lc.check_grid_search_refusals(emu_lib)


@pytest.mark.parametrize("name", SQUARE)
def test_search_between_two_frames_of_65535_features(emu_lib, name):
    lc.check_search_at_limit(emu_lib, name, n1=lc.N2_MAX)


def test_hamming_scan_of_65535_train_rows(emu_lib):
    """the FP4 kernel, one query, the best in row 65534 and the runner-up in row 32768; slices on and off"""
    import test_hamming_tracker as ht
    ht.check_limit_rows(emu_lib, first_only=True)


def test_pose_optimisation_of_65535_features(emu_lib):
    import pose_opt_checks as pk
    from orb_slam3_rgbl_amd import frontend as F
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    pk.check_limit(emu_lib, mt)
    pk.check_limit_refused(emu_lib, mt)
    mt.close()


def test_sim3_of_65535_correspondences(emu_lib):
    import sim3_checks as sk
    from orb_slam3_rgbl_amd import frontend as F
    mt = F.ORBmatcher(0.6, False, lib=emu_lib)
    sk.check_limit_n(emu_lib, mt)
    mt.close()


@pytest.mark.parametrize("name", lc.POINT_LIMIT_SEARCHES)
def test_search_of_2_to_the_20_minus_1_points(emu_lib, name):
    lc.check_point_limit(emu_lib, name)


def test_resident_frame_of_65535_features(emu_lib):
    lc.check_resident_at_limit(emu_lib)


@pytest.mark.parametrize("side", ["right", "left"])
def test_stereo_matches_with_65535_keypoints_in_one_view(emu_lib, side):
    import torch

    import stereo_cases as S
    assert S.case_limit(emu_lib, torch.device("cpu"), side) > 0


def test_the_multiplicity_model_of_the_distinctive_descriptor_agrees_with_the_oracle(oracle):
    """no kernel involved: the reference of the GPU tier's 65535-observation cases, at sizes the oracle can do"""
    assert lc.check_multiplicity_model() == 60


def test_distinctive_descriptors_refuse_65536_observations(emu_lib):
    lc.check_distinctive_refused(emu_lib)


@pytest.mark.parametrize("form", [0, 1, 2], ids=["kf_f", "kf_two_camera_f", "kf_kf"])
def test_search_by_bow_with_a_bucket_of_16384(emu_lib, form):
    lc.check_bow_at_limit(emu_lib, form)


def test_search_by_bow_refuses_a_bucket_of_16385(emu_lib):
    lc.check_bow_refused(emu_lib)


def test_depth_of_scans_around_2_to_the_20_points(emu_lib):
    lc.check_depth_index_limit(emu_lib)


def test_kfdb_batch_of_65535_queries(emu_lib):
    lc.check_kfdb_query_limit(emu_lib)


@pytest.mark.parametrize("nfeatures", [2000, 6000])
def test_extraction_from_an_image_4096_wide(emu_lib, nfeatures):
    lc.check_extractor_width_limit(emu_lib, nfeatures)


def test_extractor_refuses_sides_of_4097(emu_lib):
    lc.check_extractor_side_refused(emu_lib)


def test_extraction_with_the_longest_node_list(emu_lib):
    assert lc.check_extractor_node_list_limit(emu_lib) >= 60000
