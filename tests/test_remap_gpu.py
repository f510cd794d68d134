"""The rectification kernels (csrc/rectify.hip) on a real MI355X: every case of tests/remap_cases.py through rgbl_remap and
rgbl_remap_batch_device, bit for bit against tests/remap_ref.py (a restatement of cv::remap, unpinned); the raw-image
extraction rgbl_extract_rectified against rgbl_extract on the restated image; a raw stereo pair through two rectifiers into
rgbl_stereo_matches.  tests/test_remap_emu.py runs the same cases under the SIMT emulator first."""
import pytest
import torch

import remap_cases as RC

DEV = torch.device("cuda", 0)
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("channels", RC.CHANNELS)
@pytest.mark.parametrize("name", RC.SMALL_CASES)
def test_host_call(gpu_lib, name, channels):
    info = RC.check_host_case(gpu_lib, name, channels)
    if name == "random":
        assert info["staged_tiles"] == 0 and info["direct_tiles"] == 4
    if name == "minify":
        assert info["direct_tiles"] > 0
    if name == "mixed":
        assert info["staged_tiles"] > 0 and info["direct_tiles"] > 0
    if name in ("identity", "smooth", "wild"):
        assert info["direct_tiles"] == 0


def test_full_frame(gpu_lib):
    info = RC.check_host_case(gpu_lib, "big", 1)
    assert info["staged_tiles"] == 12 * 15 and info["direct_tiles"] == 0


@pytest.mark.parametrize("batch", [8, 9])
@pytest.mark.parametrize("channels", RC.CHANNELS)
def test_batches_with_frame_strides(gpu_lib, channels, batch):
    info = RC.check_batch_case(gpu_lib, DEV, "mixed", channels, batch)
    assert info["staged_tiles"] > 0 and info["direct_tiles"] > 0


def test_error_returns(gpu_lib):
    RC.check_errors(gpu_lib)


def test_extract_rectified_full_frame(gpu_lib):
    RC.check_extract_rectified(gpu_lib, 752, 480, 1, nfeatures=1000, nlevels=8)


@pytest.mark.parametrize("channels", [3, 4])
def test_extract_rectified_colour(gpu_lib, channels):
    RC.check_extract_rectified(gpu_lib, 320, 240, channels, nfeatures=500, nlevels=4)


def test_stereo_pair_through_two_rectifiers(gpu_lib):
    RC.check_stereo_pair(gpu_lib)
