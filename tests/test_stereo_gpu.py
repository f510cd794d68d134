"""Frame::ComputeStereoMatches on keypoint sets built by the test (tests/stereo_cases.py): the product library on a real MI355X
against the oracle, bit for bit.  tests/test_stereo_emu.py runs the same cases under the SIMT emulator."""
import pytest
import torch

import stereo_cases as S

DEV = torch.device("cuda", 0)
pytestmark = pytest.mark.gpu
# (n_left, n_right): every right count of the tile / group list with 12 and with 130 left keypoints, every left count around the
# workgroup's 64 keypoints on one, two and four tiles
NR = (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 2051, 4096, 4100, 6145)
TILES = [(nl, nr) for nl in (12, 130) for nr in NR] + [(nl, nr) for nl in (1, 63, 64, 65) for nr in (129, 2049, 6145)]


@pytest.mark.parametrize("n_left,n_right", TILES)
def test_tiles_and_groups(gpu_lib, n_left, n_right):
    assert S.case_tiles(gpu_lib, DEV, n_left, n_right) == min(n_left, n_right, 19)


@pytest.mark.parametrize("name", sorted(S.TIES))
def test_ties_go_to_the_lowest_right_index(gpu_lib, name):
    S.case_ties(gpu_lib, DEV, name)


@pytest.mark.parametrize("n_cand", [15, 16, 17, 32, 33])
def test_flush_at_exact_candidate_counts(gpu_lib, n_cand):
    S.case_flush(gpu_lib, DEV, n_cand)


def test_flush_every_right_keypoint_a_candidate(gpu_lib):
    S.case_flush_everything(gpu_lib, DEV)


@pytest.mark.parametrize("case", [S.case_gate_rows, S.case_gate_octaves, S.case_gate_u, S.case_gate_distance], ids=lambda f: f.__name__[5:])
def test_gates_at_equality(gpu_lib, case):
    assert case(gpu_lib, DEV) > 0


@pytest.mark.parametrize("case", [S.case_sad_right_border, S.case_sad_left_border, S.case_sad_rows, S.case_sad_bestinc], ids=lambda f: f.__name__[5:])
def test_sad_window(gpu_lib, case):
    assert case(gpu_lib, DEV) > 0


def test_zero_disparity(gpu_lib):
    S.case_zero_disparity(gpu_lib, DEV)


@pytest.mark.parametrize("name", sorted(S.FILTER_SMALL))
def test_filter_small_sets(gpu_lib, name):
    S.case_filter_small(gpu_lib, DEV, name)


@pytest.mark.parametrize("n_left", [2047, 2048, 2049, 2300])
def test_filter_tail(gpu_lib, n_left):
    S.case_filter_tail(gpu_lib, DEV, n_left)


def test_host_path_sizes(gpu_lib):
    S.case_host_sizes(gpu_lib, DEV)


@pytest.mark.parametrize("batch", [5, 3, 1])
def test_batch_entry_point(gpu_lib, batch):
    S.case_batch(gpu_lib, DEV, batch)


def test_batch_entry_point_ignores_stale_tile_entries(gpu_lib):
    S.case_batch_stale_tile_entries(gpu_lib, DEV)


def test_argument_errors(gpu_lib):
    S.case_argument_errors(gpu_lib, DEV)
