"""Frame::ComputeStereoMatches on keypoint sets built by the test (tests/stereo_cases.py): the kernel sources under the SIMT emulator
against the oracle, bit for bit.  tests/test_stereo_gpu.py runs the same cases on the card."""
import pytest
import torch

import stereo_cases as S

DEV = torch.device("cpu")
# (n_left, n_right): every right count of the tile / group list with 12 left keypoints, every left count around the workgroup's 64
# keypoints; the 6145 and the 4096 shape once each
TILES = [(12, n) for n in (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 2051, 4096)] + [(n, 129) for n in (1, 63, 64, 65, 130)] + \
        [(65, 4100), (130, 6145)]


@pytest.mark.parametrize("n_left,n_right", TILES)
def test_tiles_and_groups(emu_lib, n_left, n_right):
    assert S.case_tiles(emu_lib, DEV, n_left, n_right) == min(n_left, n_right, 19)


@pytest.mark.parametrize("name", sorted(S.TIES))
def test_ties_go_to_the_lowest_right_index(emu_lib, name):
    S.case_ties(emu_lib, DEV, name)


@pytest.mark.parametrize("n_cand", [15, 16, 17, 32, 33])
def test_flush_at_exact_candidate_counts(emu_lib, n_cand):
    S.case_flush(emu_lib, DEV, n_cand)


def test_flush_every_right_keypoint_a_candidate(emu_lib):
    S.case_flush_everything(emu_lib, DEV)


@pytest.mark.parametrize("case", [S.case_gate_rows, S.case_gate_octaves, S.case_gate_u, S.case_gate_distance], ids=lambda f: f.__name__[5:])
def test_gates_at_equality(emu_lib, case):
    assert case(emu_lib, DEV) > 0


@pytest.mark.parametrize("case", [S.case_sad_right_border, S.case_sad_left_border, S.case_sad_rows, S.case_sad_bestinc], ids=lambda f: f.__name__[5:])
def test_sad_window(emu_lib, case):
    assert case(emu_lib, DEV) > 0


def test_zero_disparity(emu_lib):
    S.case_zero_disparity(emu_lib, DEV)


@pytest.mark.parametrize("name", sorted(S.FILTER_SMALL))
def test_filter_small_sets(emu_lib, name):
    S.case_filter_small(emu_lib, DEV, name)


@pytest.mark.parametrize("n_left", [2047, 2048, 2049, 2300])
def test_filter_tail(emu_lib, n_left):
    S.case_filter_tail(emu_lib, DEV, n_left)


def test_host_path_sizes(emu_lib):
    S.case_host_sizes(emu_lib, DEV)


@pytest.mark.parametrize("batch", [5, 3, 1])
def test_batch_entry_point(emu_lib, batch):
    S.case_batch(emu_lib, DEV, batch)


def test_batch_entry_point_ignores_stale_tile_entries(emu_lib):
    S.case_batch_stale_tile_entries(emu_lib, DEV)


def test_argument_errors(emu_lib):
    S.case_argument_errors(emu_lib, DEV)
